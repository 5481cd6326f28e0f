"""SAFMN written from the definition in include/innfer_amd.h with torch's own CPU ops in float64, and beside it the fp16 storage model: the same forward, rounded to fp16
exactly where the engine declares a slab store, at s in front of the aggregation, and at every conv's weights.  Synthetic weights, filled once per case."""
import functools

import torch
import torch.nn.functional as F

r16 = lambda v: v.half().double()


def fill(in_ch, dim, n_blocks, ffn_scale, scale, seed):
    """A SAFMN state dict (float32) with weights of a size that keeps every activation O(1)."""
    from innfer_amd import synth
    from innfer_amd.architectures.keys import safmn_shapes
    sd = {}
    for i, (k, shp) in enumerate(safmn_shapes(dim, n_blocks, ffn_scale, scale, in_ch).items()):
        fan = 1 if len(shp) == 1 else shp[1] * shp[2] * shp[3]
        lo, hi = (0.5, 1.5) if 'norm' in k and k.endswith('weight') else (-1.0, 1.0)
        amp = 1.0 if 'norm' in k else (0.2 if k.endswith('bias') else 1.5 / fan ** 0.5)
        sd[k] = torch.from_numpy(synth.uniform(shp, 9100 + 37 * seed + i, lo, hi)) * amp
    return sd


def safm(u, mfr_w, mfr_b, aggr_w, aggr_b, model=False):
    """GELU(aggr(cat(s_0 .. s_3))) * u in float64; u [N, dim, H, W], mfr_w [dim, 1, 3, 3].  model: s and aggr's weight rounded to fp16."""
    h, w = u.shape[2:]
    chunk = u.shape[1] // 4
    s = []
    for i in range(4):
        c = slice(i * chunk, (i + 1) * chunk)
        p = u[:, c] if i == 0 else F.adaptive_max_pool2d(u[:, c], (h >> i, w >> i))
        p = F.conv2d(p, mfr_w[c], mfr_b[c], padding=1, groups=chunk)
        s.append(p if i == 0 else F.interpolate(p, size=(h, w), mode='nearest'))
    s = torch.cat(s, 1)
    if model:
        s, aggr_w = r16(s), r16(aggr_w)
    return F.gelu(F.conv2d(s, aggr_w, aggr_b)) * u


def forward(sd, x, model=False):
    """The network in float64 on an fp16-representable input; model: the storage model."""
    q = r16 if model else (lambda v: v)
    p = {k: v.double() for k, v in sd.items()}
    wt = lambda k: q(p[k + '.weight'])
    ln = lambda t, k: F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), p[k + '.weight'], p[k + '.bias'], 1e-6).permute(0, 3, 1, 2)
    f0 = q(F.conv2d(x.double(), wt('to_feat'), p['to_feat.bias'], padding=1))
    t, b = f0, 0
    while f'feats.{b}.norm1.weight' in p:
        k = f'feats.{b}.'
        u = q(ln(t, k + 'norm1'))
        mw, mb = torch.cat([p[k + f'safm.mfr.{i}.weight'] for i in range(4)]), torch.cat([p[k + f'safm.mfr.{i}.bias'] for i in range(4)])
        t = q(t + safm(u, mw, mb, p[k + 'safm.aggr.weight'], p[k + 'safm.aggr.bias'], model))
        u = q(ln(t, k + 'norm2'))
        hid = q(F.gelu(F.conv2d(u, wt(k + 'ccm.ccm.0'), p[k + 'ccm.ccm.0.bias'], padding=1)))
        t = q(t + F.conv2d(hid, wt(k + 'ccm.ccm.2'), p[k + 'ccm.ccm.2.bias']))
        b += 1
    y = q(F.conv2d(q(t + f0), wt('to_img.0'), p['to_img.0.bias'], padding=1))
    return F.pixel_shuffle(y, int(round((y.shape[1] / x.shape[1]) ** 0.5)))


# name -> (in_ch, dim, n_blocks, scale, input shape, seed)
FIXTURES = {"dim36 2 blocks x2": (3, 36, 2, 2, (1, 3, 24, 40), 1), "dim128 1 block x4": (3, 128, 1, 4, (1, 3, 19, 33), 2), "gray x3": (1, 36, 1, 3, (2, 1, 17, 22), 3)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(state dict, input, float64 result, storage model's result) of a fixture, computed once."""
    from innfer_amd import synth
    in_ch, dim, nb, s, shape, seed = FIXTURES[name]
    sd = fill(in_ch, dim, nb, 2.0, s, seed)
    x = torch.from_numpy(synth.uniform(shape, 9000 + seed)).half()
    return sd, x, forward(sd, x), forward(sd, x, model=True)
