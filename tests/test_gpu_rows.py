"""GPU tests of addk_gather_rows (csrc/rows.hip) through the C ABI: every row size and alignment class of its contract against torch
indexing, byte for byte, with canary bytes around every destination row."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROW_BYTES = (1, 3, 16, 4 * (33 * 65 * 24), 129 * 257)       # bytes; a level-3 row of 24 channels and a label row among them
# (source offset, destination offset) inside a 16-byte line: both aligned (16-byte accesses from the first byte), the same odd offset
# (16-byte accesses behind a head of single bytes), the same offset inside a word only (4-byte accesses), nothing shared (bytes)
OFFSETS = ((0, 0), (5, 5), (4, 8), (1, 2))
SRC_ROWS, DST_ROWS, PAD = 5, 8, 64
MODES = ('identity', 'permutation', 'null', 'null_src', 'null_dst')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _data(dev):
    """Per item (row size x alignment class): its source bytes [SRC_ROWS rows] and a destination pattern [DST_ROWS rows] inside
    allocations with PAD + offset bytes in front and PAD behind, made once and never modified."""
    gen = torch.Generator().manual_seed(5)
    items = []
    for rb in ROW_BYTES:
        for so, do in OFFSETS:
            src = torch.randint(0, 256, (PAD + so + SRC_ROWS * rb + PAD,), dtype=torch.uint8, generator=gen).to(dev)
            dst = torch.randint(0, 256, (PAD + do + DST_ROWS * rb + PAD,), dtype=torch.uint8, generator=gen).to(dev)
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            items.append((rb, so, do, src, dst))
    return items


def _indices(mode, n):
    src = {'identity': list(range(n)), 'permutation': [3, 0, 4, 1][:n], 'null': None, 'null_src': None, 'null_dst': [4, 2, 0, 3][:n]}[mode]
    dst = {'identity': list(range(n)), 'permutation': [6, 1, 4, 3][:n], 'null': None, 'null_src': [5, 0, 7, 2][:n], 'null_dst': None}[mode]
    return src, dst


def _launch(lib, L, dev, items, dsts, src_row, dst_row, n):
    arr = (L.RowsItem * len(items))()
    for it, (rb, so, do, src, _), dst in zip(arr, items, dsts):
        it.src, it.dst, it.row_bytes = src.data_ptr() + PAD + so, dst.data_ptr() + PAD + do, rb
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    sr = None if src_row is None else torch.tensor(src_row, dtype=torch.int32, device=dev)
    dr = None if dst_row is None else torch.tensor(dst_row, dtype=torch.int32, device=dev)
    a = L.GatherRowsArgs()
    a.items, a.nitems, a.nrows = table.data_ptr(), len(items), n
    a.src_row, a.dst_row = (None if sr is None else sr.data_ptr()), (None if dr is None else dr.data_ptr())
    rc = lib.addk_gather_rows(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('mode', MODES)
def test_gather_rows_matches_torch_indexing(dev, mode):
    """ONE launch moves every item (5 row sizes x 4 alignment classes), nrows 1..4: the destination rows hold the source rows torch
    indexing selects, every other byte of the destination allocations (the rows not named, the bytes in front and behind) keeps its
    pattern, and a second launch leaves the same bytes."""
    import addk._lib as L
    lib = L.load()
    items = _data(dev)
    for n in (1, 2, 3, 4):
        src_row, dst_row = _indices(mode, n)
        want, dsts = [], []
        for rb, so, do, src, dst in items:
            rows = src[PAD + so:PAD + so + SRC_ROWS * rb].view(SRC_ROWS, rb)[list(range(n)) if src_row is None else src_row]
            w = dst.clone()
            w[PAD + do:PAD + do + DST_ROWS * rb].view(DST_ROWS, rb)[list(range(n)) if dst_row is None else dst_row] = rows
            assert rb < 16 or not torch.equal(w, dst)           # (a random row of 1 or 3 bytes may equal the pattern it replaces)
            want.append(w)
            dsts.append(dst.clone())
        assert _launch(lib, L, dev, items, dsts, src_row, dst_row, n) == 0
        for (rb, so, do, _, _), w, d in zip(items, want, dsts):
            assert torch.equal(d, w), (mode, n, rb, so, do, int((d != w).sum()))
        assert _launch(lib, L, dev, items, dsts, src_row, dst_row, n) == 0
        assert all(torch.equal(d, w) for w, d in zip(want, dsts))


def test_gather_rows_refuses_what_it_does_not_take(dev):
    """An error code and no launch: the destinations keep their pattern."""
    import addk
    import addk._lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    items = [it for it in _data(dev) if it[0] == 16][:2]
    dsts = [it[4].clone() for it in items]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(d, it[4]) for d, it in zip(dsts, items))

    assert _launch(lib, L, dev, items, dsts, None, None, 0) != 0 and untouched()                 # nrows < 1
    assert _launch(lib, L, dev, items, dsts, None, None, -3) != 0 and untouched()
    for bad in ('row_bytes', 'src', 'dst'):
        arr = (L.RowsItem * 2)()
        for i, (it, (rb, so, do, src, _), dst) in enumerate(zip(arr, items, dsts)):
            it.src, it.dst, it.row_bytes = src.data_ptr() + PAD, dst.data_ptr() + PAD, rb
            if i == 1:
                setattr(it, bad, 0)
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        a = L.GatherRowsArgs()
        a.items, a.nitems, a.nrows = table.data_ptr(), 2, 2
        rc = lib.addk_gather_rows(C.byref(a), st)
        assert rc != 0 and untouched(), bad                                                           # the good first item did not run either
        with pytest.raises(addk.AddkError):
            L.check(rc, 'gather_rows')
        a.nitems = 0
        assert lib.addk_gather_rows(C.byref(a), st) != 0 and untouched()                            # nitems < 1
    # more units of 16 KiB than a launch indexes: refused from the table alone
    arr = (L.RowsItem * 1)()
    arr[0].src, arr[0].dst, arr[0].row_bytes = items[0][3].data_ptr() + PAD, dsts[0].data_ptr() + PAD, 16385
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    a = L.GatherRowsArgs()
    a.items, a.nitems, a.nrows = table.data_ptr(), 1, 2 ** 31 - 1
    assert lib.addk_gather_rows(C.byref(a), st) != 0 and untouched()
    arr[0].row_bytes = 2 ** 62
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    a.items, a.nrows = table.data_ptr(), 1
    assert lib.addk_gather_rows(C.byref(a), st) != 0 and untouched()
    assert lib.addk_gather_rows(C.byref(L.GatherRowsArgs()), st) != 0                               # null pointers
    assert lib.addk_gather_rows(None, st) != 0
    assert _launch(lib, L, dev, items, dsts, None, None, 2) == 0 and not untouched()                # ... and the same arguments, valid, do run
