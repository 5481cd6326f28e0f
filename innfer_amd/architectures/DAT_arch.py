"""DAT shell (Chen et al. 2023: "Dual Aggregation Transformer for Image Super-Resolution"; DAT, DAT-S, DAT-2, DAT-light and their fine-tunes).
The reference has no such architecture; constructor surface and state-dict keys are the published ones (dat_arch.py; keys.dat_shapes is the one table), the graph is built
inside libinnfer_amd.so (csrc/net.hip, kind 8; csrc/win_attn_rect.hip, chan_self_attn.hip, dwconv.hip, aim_mix.hip, chan_attn.hip's GELU excite, layer_norm.hip).

With C = embed_dim, nH heads of d = C / nH, split = [s0, s1], hid = int(C * expansion_factor), tokens = pixels of the H x W grid (NO padding of the image):

    forward(x):   f = conv_first(x - mean); f = conv_after_body(norm(RGs(before_RG.1(f)))) + f; tail (pixelshuffle | pixelshuffledirect); + mean      (mean, img_range 1: as SwinIR)
    RG i:         t = conv(blocks(t)) + t
    block b:      t = t + attn(norm1(t));  t = t + ffn(norm2(t));   even b: attention over rectangular windows (ASA), odd b: across channels (ACA)
    ASA:          qkv = Linear(C, 3 C)(u), zero-padded behind the Linear to multiples of max(s0, s1); heads [0, nH/2) windows s0 x s1, heads [nH/2, nH) s1 x s0; shifted blocks
                  use the windows of the rolled frame and a -100 mask; softmax((q d^-0.5) k^T + B_h + M) v; B_h from a DynamicPosBias MLP per branch
    ACA:          per head softmax_y(temperature_h <q^[:, x], k^[:, y]>) v over all pixels, q^ = F.normalize over the pixels
    both:         c = GELU(BN(dwconv3x3(v)));  out = proj(X sigmoid(cm(mean_pixels(Y))) + Y sigmoid(sm(X))),  (X, Y) = (a, c) for ASA, (c, a) for ACA
    ffn:          h = GELU(fc1(u)); x1, x2 = halves; fc2(x1 * dwconv3x3(LayerNorm(hid / 2)(x2)))

Everything below happens at load, in float64 or float32, before the engine's one fp16 rounding: the dense bias tables are evaluated in float64 from the DynamicPosBias
weights and rounded once to float32; every BatchNorm is folded into the conv in front of it; qkv / proj are re-laid-out as SwinIR's (an ACA block's q rows carry no
d^-0.5); the depthwise conv and the two interaction MLPs are permuted to the head-padded channel order (channel 32 h + e = model channel d h + e); fc1's rows are laid
out so that x1 and x2 each own a block padded to a multiple of 64, fc2's columns to match; `temperature` is passed as is."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import dat_pos_dim, dat_shapes
from .SwinIR_arch import RGB_MEAN, SwinIR, pad64, relayout

SPLITS = ((8, 32), (8, 16))
_TAILS = {'pixelshuffle': 0, 'pixelshuffledirect': 1}


def shifted_blocks(depths):
    """(i, b) of the blocks whose windows are those of the rolled frame, by the published rule; only even b (the window form) matter."""
    return [(i, b) for i, depth in enumerate(depths) for b in range(depth)
            if b % 2 == 0 and ((i % 2 == 0 and b > 0 and (b - 2) % 4 == 0) or (i % 2 != 0 and b % 4 == 0))]


def rpe_biases(wh, ww):
    """[(2 wh - 1)(2 ww - 1), 2] float64: the integer offsets (dy, dx), dy-major -- the published buffer."""
    dy, dx = torch.meshgrid(torch.arange(1 - wh, wh), torch.arange(1 - ww, ww), indexing='ij')
    return torch.stack([dy.reshape(-1), dx.reshape(-1)], 1).double()


def relative_position_index(wh, ww):
    """[T, T] long: (ri - rj + wh - 1)(2 ww - 1) + (ci - cj + ww - 1) for tokens row-major in a wh x ww window -- the published buffer."""
    r, c = torch.arange(wh * ww) // ww, torch.arange(wh * ww) % ww
    return (r[:, None] - r[None, :] + wh - 1) * (2 * ww - 1) + (c[:, None] - c[None, :] + ww - 1)


def dynamic_pos_bias(sd, prefix, rel):
    """pos3(pos2(pos1(pos_proj(rel)))) in float64, pos1 = pos2 = [LayerNorm, ReLU, Linear], pos3 likewise: [rows, nH / 2]."""
    f = lambda k: sd[prefix + k].detach().double().cpu()
    x = rel.double() @ f('pos_proj.weight').T + f('pos_proj.bias')
    for m in ('pos1', 'pos2', 'pos3'):
        x = torch.nn.functional.layer_norm(x, (x.shape[-1],), f(m + '.0.weight'), f(m + '.0.bias'), 1e-5)
        x = torch.relu(x) @ f(m + '.2.weight').T + f(m + '.2.bias')
    return x


def dense_bias(sd, block_prefix, s0, s1, rpe=None):
    """The dense [nH, T, T] float32 table of an ASA block: per branch B[h][i][j] = pos(rel)[index[i][j]][h], evaluated in float64 and rounded once.  rpe: a checkpoint's
    stored rpe_biases per branch (authoritative when given)."""
    out = []
    for br, (wh, ww) in enumerate(((s0, s1), (s1, s0))):
        rel = rpe_biases(wh, ww) if rpe is None or rpe[br] is None else torch.as_tensor(rpe[br]).double()
        if tuple(rel.shape) != ((2 * wh - 1) * (2 * ww - 1), 2):
            raise NotImplementedError(f'DAT: rpe_biases of shape {tuple(rel.shape)} for a {wh} x {ww} window ({((2 * wh - 1) * (2 * ww - 1), 2)})')
        pos = dynamic_pos_bias(sd, f'{block_prefix}attn.attns.{br}.pos.', rel)
        idx = relative_position_index(wh, ww)
        out.append(pos[idx.reshape(-1)].reshape(wh * ww, wh * ww, -1).permute(2, 0, 1))
    return np.ascontiguousarray(torch.cat(out, 0).float().numpy())


def fold_bn(w, b, sd, bn, eps=1e-5):
    """BatchNorm2d (eval) `bn` behind a conv with weight w [K, ...] and bias b [K], folded into both (float64)."""
    f = lambda k: sd[bn + k].detach().double().cpu()
    g = f('.weight') / torch.sqrt(f('.running_var') + eps)
    return w * g.reshape(-1, *([1] * (w.dim() - 1))), (b - f('.running_mean')) * g + f('.bias')


def head_pad_index(Cc, nH):
    """Model channel c = d h + e -> 32 h + e."""
    d = Cc // nH
    c = torch.arange(Cc)
    return 32 * (c // d) + c % d


def fc_halves(w1, b1, w2, b2, Cc, hid):
    """fc1 [hid, C] / fc2 [C, hid / 2] -> fc1 rows as [x1 | pad | x2 | pad] (each block h1p = pad64(hid / 2)) over C_pad columns, fc2 as [C_pad, h1p]: float32 numpy."""
    half, h1p, Cp = hid // 2, pad64(hid // 2), pad64(Cc)
    wo, bo = np.zeros((2 * h1p, Cp, 1, 1), np.float32), np.zeros(2 * h1p, np.float32)
    wo[:half, :Cc, 0, 0], wo[h1p:h1p + half, :Cc, 0, 0] = w1[:half], w1[half:]
    bo[:half], bo[h1p:h1p + half] = b1[:half], b1[half:]
    w2o, b2o = np.zeros((Cp, h1p, 1, 1), np.float32), np.zeros(Cp, np.float32)
    w2o[:Cc, :half, 0, 0] = w2
    b2o[:Cc] = b2
    return wo, bo, w2o, b2o


def qkv_unscaled(w, b, Cc, nH):
    """attn.qkv of a channel-attention block in SwinIR's head-padded row order (group which nH + h, 32 rows each), WITHOUT d^-0.5 in the q rows: float32 numpy."""
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    d, rows = Cc // nH, (3 * nH + 1) // 2 * 64
    wo, bo = np.zeros((rows, pad64(Cc), 1, 1), np.float32), np.zeros(rows, np.float32)
    for which in range(3):
        for h in range(nH):
            src = slice(which * Cc + h * d, which * Cc + (h + 1) * d)
            dst = slice((which * nH + h) * 32, (which * nH + h) * 32 + d)
            wo[dst, :Cc, 0, 0], bo[dst] = w[src], b[src]
    return wo, bo


class DAT(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, in_chans=3, embed_dim=180, split_size=(2, 4), depth=(2, 2, 2, 2), num_heads=(2, 2, 2, 2), expansion_factor=4., qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, use_chk=False, upscale=2, img_range=1., resi_connection='1conv', upsampler='pixelshuffle',
                 pos_dim=None, shift_blocks=None, rpe_biases=None, **unused):
        depths = list(depth)
        heads = list(num_heads) if isinstance(num_heads, (list, tuple)) else [num_heads] * len(depths)
        nh = heads[0] if heads else 0
        split = tuple(split_size) if isinstance(split_size, (list, tuple)) else (split_size,)
        ok_c = isinstance(embed_dim, int) and embed_dim >= 1
        hidden = int(embed_dim * expansion_factor) if ok_c else 0
        unsupported = []
        if split not in SPLITS: unsupported.append(f'split_size={list(split)} ([8, 32], [8, 16])')
        if not depths or any(not isinstance(d, int) or d < 1 for d in depths): unsupported.append(f'depth={depths}')
        if len(heads) != len(depths) or any(h != nh for h in heads): unsupported.append(f'num_heads={heads} (one count for every residual group)')
        elif not (ok_c and 16 <= embed_dim <= 256 and isinstance(nh, int) and nh in (2, 4, 6, 8) and embed_dim % nh == 0 and embed_dim // nh <= 32):
            unsupported.append(f'embed_dim={embed_dim}, num_heads={nh} (embed_dim 16 .. 256, an even number of <= 8 heads of <= 32 channels, embed_dim % num_heads == 0)')
        if not (2 <= hidden <= 1024 and hidden % 2 == 0): unsupported.append(f'expansion_factor={expansion_factor} (int(embed_dim * expansion_factor) = {hidden}; built: even, <= 1024)')
        if not qkv_bias: unsupported.append('qkv_bias=False')
        if qk_scale is not None: unsupported.append(f'qk_scale={qk_scale} (None: head_dim ** -0.5)')
        if img_range != 1: unsupported.append(f'img_range={img_range} (1)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if upsampler not in _TAILS: unsupported.append(f'upsampler={upsampler!r} (pixelshuffle, pixelshuffledirect)')
        elif upscale not in (2, 3, 4): unsupported.append(f'upscale={upscale} (2, 3, 4)')
        if resi_connection not in ('1conv', '3conv'): unsupported.append(f'resi_connection={resi_connection!r}')
        if unsupported:
            raise NotImplementedError('DAT option(s) not built on the HIP path: ' + ', '.join(unsupported))
        self_pos = dat_pos_dim(embed_dim) if pos_dim is None else int(pos_dim)
        EngineModule.__init__(self, dat_shapes(in_chans, embed_dim, depths, nh, expansion_factor, upscale, upsampler, resi_connection, self_pos))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.num_heads, self.hidden, self.upscale = embed_dim, depths, nh, hidden, upscale
        self.upsampler, self.resi_connection, self.n_blocks, self.split, self.pos_dim = upsampler, resi_connection, sum(depths), split, self_pos
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans
        # which blocks shift: a checkpoint's stored masks decide when the loader hands them over, else the published rule
        sb = shifted_blocks(depths) if shift_blocks is None else [tuple(int(v) for v in q) for q in shift_blocks]
        bad = [q for q in sb if len(q) != 2 or not (0 <= q[0] < len(depths) and 0 <= q[1] < depths[q[0]] and q[1] % 2 == 0)]
        if bad:
            raise NotImplementedError(f'DAT: shift_blocks {bad} do not name window blocks (even index) of depth={depths}')
        self.shift_blocks = sorted(set(sb))
        self.rpe = None if rpe_biases is None else [None if r is None else np.asarray(r, np.float64) for r in rpe_biases]
        if self.rpe is not None:
            for br, (wh, ww) in enumerate(((split[0], split[1]), (split[1], split[0]))):
                if self.rpe[br] is not None and self.rpe[br].shape != ((2 * wh - 1) * (2 * ww - 1), 2):
                    raise NotImplementedError(f'DAT: rpe_biases of shape {self.rpe[br].shape} for a {wh} x {ww} window')

    def _blocks(self):
        return [(i, j) for i, depth in enumerate(self.depths) for j in range(depth)]

    def _create_handle(self):
        h = C.c_void_p()
        depths = (C.c_int * len(self.depths))(*self.depths)
        mean = (C.c_float * 4)(*self.mean)
        flags = [int((i, j) in self.shift_blocks) for i, j in self._blocks()]
        shift = (C.c_int * len(flags))(*flags)
        L.check(L.lib.innfer_dat_create(C.byref(h), self.in_nc, self.out_nc, self.nf, depths, len(self.depths), self.num_heads, self.hidden, self.split[0], self.split[1],
                                        _TAILS[self.upsampler], self.upscale, int(self.resi_connection == '3conv'), mean, shift))
        return h

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: qkv (an ACA block's q rows unscaled), proj and the skeleton's convs through SwinIR's relayout; fc1 / fc2 in halves."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()
            w, b = EngineModule._conv_tensors(self, base, sd)
            if base.endswith('ffn.fc1') or base.endswith('ffn.fc2'):
                blk = base.rsplit('.', 1)[0]
                f32 = lambda key: sd[key].detach().float().cpu().numpy()
                w1, b1, w2, b2 = fc_halves(f32(blk + '.fc1.weight'), f32(blk + '.fc1.bias'), f32(blk + '.fc2.weight'), f32(blk + '.fc2.bias'), self.nf, self.hidden)
                cache[base] = (w1, b1) if base.endswith('fc1') else (w2, b2)
            elif base.endswith('attn.qkv') and int(base.split('.')[3]) % 2 == 1:          # ACA: q and k are normalised, there is no d^-0.5
                cache[base] = qkv_unscaled(w, b, self.nf, self.num_heads)
            else:
                cache[base] = relayout(base, w, b, self.nf, self.num_heads, self.hidden, self.in_nc, self.upscale, self.upsampler == 'pixelshuffledirect')
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def block_params(self, sd, i, j):
        """The array innfer_net_set_dat_block takes for block (i, j), float32, in the header's order; everything folded and permuted in float64."""
        Cc, nH, half = self.nf, self.num_heads, self.hidden // 2
        chp, hc, hs = 32 * nH, Cc // 8, Cc // 16
        b = f'layers.{i}.blocks.{j}.'
        f = lambda k: sd[b + k].detach().double().cpu()
        hp = head_pad_index(Cc, nH)

        def rows(x):                                     # [C, ...] -> [Chp, ...]
            o = torch.zeros((chp,) + tuple(x.shape[1:]), dtype=torch.float64)
            o[hp] = x
            return o

        def cols(x):                                     # [K, C] -> [K, Chp]
            o = torch.zeros((x.shape[0], chp), dtype=torch.float64)
            o[:, hp] = x
            return o
        dw_w, dw_b = fold_bn(f('attn.dwconv.0.weight').reshape(Cc, 9), f('attn.dwconv.0.bias'), sd, b + 'attn.dwconv.1')
        ci_w1, ci_b1 = fold_bn(f('attn.channel_interaction.1.weight').reshape(hc, Cc), f('attn.channel_interaction.1.bias'), sd, b + 'attn.channel_interaction.2')
        ci_w2, ci_b2 = f('attn.channel_interaction.4.weight').reshape(Cc, hc), f('attn.channel_interaction.4.bias')
        si_w1, si_b1 = fold_bn(f('attn.spatial_interaction.0.weight').reshape(hs, Cc), f('attn.spatial_interaction.0.bias'), sd, b + 'attn.spatial_interaction.1')
        si_w2, si_b2 = f('attn.spatial_interaction.3.weight').reshape(hs), f('attn.spatial_interaction.3.bias').reshape(1)
        temp = f('attn.temperature').reshape(nH) if j % 2 else torch.zeros(nH, dtype=torch.float64)
        parts = [rows(dw_w), rows(dw_b), cols(ci_w1), ci_b1, rows(ci_w2), rows(ci_b2), cols(si_w1), si_b1, si_w2, si_b2,
                 f('ffn.sg.norm.weight'), f('ffn.sg.norm.bias'), f('ffn.sg.conv.weight').reshape(half, 9), f('ffn.sg.conv.bias'), temp]
        return np.ascontiguousarray(torch.cat([q.reshape(-1) for q in parts]).float().numpy())

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        f32 = lambda key: np.ascontiguousarray(sd[key].detach().float().cpu().numpy())
        norms = ['before_RG.1']
        n = L.lib.innfer_dat_block_floats(self._handle)
        for blk, (i, j) in enumerate(self._blocks()):
            b = f'layers.{i}.blocks.{j}.'
            norms += [b + 'norm1', b + 'norm2']
            if j % 2 == 0:
                table = dense_bias(sd, b, self.split[0], self.split[1], self.rpe)
                L.check(L.lib.innfer_net_set_attn_bias(self._handle, blk, table.ctypes.data))
            prm = self.block_params(sd, i, j)
            if prm.size != n:
                raise RuntimeError(f'DAT: block ({i}, {j}) packs {prm.size} floats, the engine takes {n}')
            L.check(L.lib.innfer_net_set_dat_block(self._handle, blk, prm.ctypes.data, n))
        norms.append('norm')
        for idx, key in enumerate(norms):
            g, be = f32(key + '.weight'), f32(key + '.bias')
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, be.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'DAT is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        """Any H x W: the engine pads nothing (the windows' frame exists only as coordinates)."""

    def forward(self, x, outm=None, out=None):
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'DAT has no outm ({outm!r})')
        return super().forward(x, None, out)
