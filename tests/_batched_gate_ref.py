"""What tests/test_gpu_batched_gate.py and its measurement share: the model, the seeded inputs and the single-image references."""
import functools

import torch
import torch.nn as nn

from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor

H, W = 129, 257
ARCH = {'c2': ARCH_C2, 'c3': ARCH_C3}
# (first seed, contrast per image).  The CPU oracle's entropies of the gated exits on these inputs (fp32, the model below):
#   c2  exit 0: 0.4654 0.4251 0.2682 0.1514                -> largest gap 0.157 between images 1 and 2
#   c3  exit 0: 0.2228 0.1041 0.0581; exit 1: 0.7657 0.4705 0.2400 -> image 2 leaves at gate 0, image 1 at gate 1, image 0 stays
INPUTS = {'c2': (21, (0.25, 0.5, 1.0, 2.0)), 'c3': (22, (2.0, 4.0, 8.0))}


def model(cfg, dev):
    """tests/test_gpu_gate.py's model (F = 20, fill_params(m, 12)) with its gated logits brought into the range where a gate can tell
    images apart.  As filled, the logits of the exits are 1e4 .. 1e7 (the dense trunk grows by a factor of several hundred from exit to
    exit), every prediction is saturated and every entropy lies in [0, 6e-4] whatever the input — measured with the CPU oracle on white
    noise of contrast 0 .. 100 and on smooth images — so no two gate values can be 1e-3 apart.  Two scalings, nothing else changes: the
    classifier shared by all exits (decoder._conv[7], weight and bias) by 2^-15 (config 2) / 2^-10 (config 3) brings exit 0 to logits of
    order 10; config 3 only: the BatchNorm affine (weight, bias) of every BatchNorm inside cell 7 by 2^-4 does the same for exit 1, whose
    feature that cell writes.  The final exit is not gated and stays saturated."""
    from addk.modeling.ADD import ADD
    arch = ARCH[cfg]
    m = ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), arch['low_level_layer'])
    fill_params(m, 12)
    with torch.no_grad():
        s = 2.0 ** (-15 if cfg == 'c2' else -10)
        m.decoder._conv[7].weight.mul_(s)
        m.decoder._conv[7].bias.mul_(s)
        if cfg == 'c3':
            for mod in m.cells[7].modules():
                if isinstance(mod, nn.BatchNorm2d):
                    mod.weight.mul_(2.0 ** -4)
                    mod.bias.mul_(2.0 ** -4)
    return m.to(dev).eval()


def inputs(cfg, dev):
    seed, contrast = INPUTS[cfg]
    return torch.cat([rand_tensor(seed + i, 'bgx', (1, 3, H, W)) * c for i, c in enumerate(contrast)]).to(dev)


@functools.lru_cache(maxsize=None)
def setup(cfg, dev):
    """(model, inputs) of one configuration, made once"""
    return model(cfg, dev), inputs(cfg, dev)


@functools.lru_cache(maxsize=None)
def singles(cfg, dev):
    """Per image, what the single-image path gives: `values` [N][gates] (Python floats) and `maps` [N][exits] (uint8 [H,W] clones), made
    once.  Exit 0 and the final exit come from ADD.dynamic_inference(output='labels') at a forcing / forbidding threshold; a middle
    exit (config 3) cannot be reached with ONE threshold when its value lies above exit 0's, so its map is read from the same cached
    single-image plan by running its segments, as tests/test_gpu_gate.py does."""
    m, X = setup(cfg, dev)
    gates = m.num_exits() - 1
    values, maps = [], []
    with torch.no_grad():
        for i in range(X.shape[0]):
            x = X[i:i + 1]
            y0, early, _, v0 = m.dynamic_inference(x, float('inf'), confidence='entropy', output='labels')
            assert early == 1
            vs, ms = [v0], [y0[0].clone()]
            plan = m._gate_plan(x, 'entropy', 'labels', None)
            for k in range(1, gates):
                plan.x_static.copy_(x)
                pos = 0
                for j in range(k + 1):
                    plan._seg(pos, plan.head_rng[j][0])
                    pos = plan.head_rng[j][1]
                torch.cuda.synchronize()
                vs.append(float(plan._conf_host[0]) * plan.heads[k].gate_scale)
                ms.append(plan.heads[k].y[0].clone())
            yf, early, _, vl = m.dynamic_inference(x, float('-inf'), confidence='entropy', output='labels')
            assert early == 0 and vl == vs[-1]
            ms.append(yf[0].clone())
            values.append(vs)
            maps.append(ms)
    return values, maps
