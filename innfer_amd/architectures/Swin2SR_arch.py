"""Swin2SR shell (Conde et al. 2022: the SwinV2 transformer for super-resolution; the classical, lightweight and real-world forms).
The reference has no such architecture; constructor surface and state-dict keys are the published ones (network_swin2sr.py), the graph is built inside libinnfer_amd.so
(csrc/net.hip, kind 7; the COS form of csrc/win_attn.hip, the ADD form of csrc/layer_norm.hip, act 12 of csrc/conv3x3.hip).  SwinIR's skeleton (SwinIR_arch.py: pad, mean,
conv_first, patch_embed.norm, RSTB = conv(blocks(t)) + t, norm, conv_after_body + f, tails, crop, shift 4 for odd j, the -100 mask) around another block:

    block j:   t = t + norm1(proj(attn(t)));  t = t + norm2(fc2(GELU(fc1(t))))          (the norm comes AFTER the branch; attn reads t itself)
    attn(t):   8 x 8 windows of roll(t, (-shift, -shift)); qkv = Linear(C, 3 C, bias=False)(t') + cat(q_bias, zeros(C), v_bias) -- k has no bias; per head h
               S = (q^ k^^T) tau_h + B_h + M,  q^ = q / max(||q||_2, 1e-12), k^ likewise;  tau_h = exp(min(logit_scale[h], ln 100));  softmax(S) v.  No d^-0.5.
    B_h:       T[225][nH] = cpb_mlp(coords), cpb_mlp = Linear(2, hidden, bias) -> ReLU -> Linear(hidden, nH, no bias);
               coords[15 a + b] = (g(a - 7), g(b - 7)), g(c) = sign(c) log2(|8 c / 7| + 1) / 3;  B_h[i][j] = 16 sigmoid(T[(ri - rj + 7) 15 + (ci - cj + 7)][h])

Load-time work, all of it in float32 or better, before the engine's one fp16 rounding: SwinIR's relayout for every tensor that is SwinIR's; attn.qkv's rows permuted to
(q | k | v) x head x 32 WITHOUT the d^-0.5 fold, its bias cat(q_bias, 0, v_bias) under the same permutation; the dense [nH][64][64] bias evaluated in float64 and rounded
once to float32 (innfer_net_set_attn_bias); tau per head in float32 (innfer_net_set_attn_scale).  A checkpoint's relative_coords_table, when stored, feeds cpb_mlp in place
of the formula for g (coords_table)."""
import ctypes as C
import math

import numpy as np

from .. import lib as L
from .engine_module import EngineModule
from .keys import swin2sr_shapes
from .SwinIR_arch import _TAILS, RGB_MEAN, SwinIR, pad64, relative_position_index, relayout

LOGIT_MAX = math.log(100.0)


def relative_coords(ws=8):
    """[(2 ws - 1)^2, 2] float64: row 15 a + b = (g(a - 7), g(b - 7)), g(c) = sign(c) log2(|8 c / (ws - 1)| + 1) / log2(8) -- the published relative_coords_table."""
    c = np.arange(-(ws - 1), ws, dtype=np.float64) / (ws - 1) * 8.0
    g = np.sign(c) * np.log2(np.abs(c) + 1.0) / 3.0
    return np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)


def cpb_bias(w0, b0, w2, coords=None, ws=8):
    """The dense [nH, ws^2 (query), ws^2 (key)] float32 table the attention kernel reads: 16 sigmoid(cpb_mlp(coords)) gathered by the relative position index; evaluated in
    float64 and rounded once.  coords: a stored relative_coords_table (any shape that flattens to [(2 ws - 1)^2, 2]) or None for the formula."""
    xy = relative_coords(ws) if coords is None else np.asarray(coords, np.float64).reshape(-1, 2)
    hid = np.maximum(xy @ np.asarray(w0, np.float64).T + np.asarray(b0, np.float64), 0.0)
    t = 16.0 / (1.0 + np.exp(-(hid @ np.asarray(w2, np.float64).T)))                    # [(2 ws - 1)^2, nH]
    return np.ascontiguousarray(t[relative_position_index(ws).numpy().reshape(-1)].reshape(ws * ws, ws * ws, -1).transpose(2, 0, 1).astype(np.float32))


def attn_scale(logit_scale):
    """exp(min(logit_scale, ln 100)) per head, float32."""
    return np.ascontiguousarray(np.exp(np.minimum(np.asarray(logit_scale, np.float64).reshape(-1), LOGIT_MAX)).astype(np.float32))


def relayout_qkv(w, q_bias, v_bias, C_, nh):
    """attn.qkv of Swin2SR for the engine: rows (q | k | v) x head x d -> group (which nh + h), 32 rows each, NO scale; bias cat(q_bias, 0, v_bias) likewise.  Index work only."""
    w = np.asarray(w, np.float32)
    b = np.concatenate([np.asarray(q_bias, np.float32), np.zeros(C_, np.float32), np.asarray(v_bias, np.float32)])
    d, rows = C_ // nh, (3 * nh + 1) // 2 * 64
    wo, bo = np.zeros((rows, pad64(C_), 1, 1), np.float32), np.zeros(rows, np.float32)
    for which in range(3):
        for h in range(nh):
            src = slice(which * C_ + h * d, which * C_ + (h + 1) * d)
            dst = slice((which * nh + h) * 32, (which * nh + h) * 32 + d)
            wo[dst, :C_, 0, 0] = w[src]
            bo[dst] = b[src]
    return wo, bo


class Swin2SR(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7, mlp_ratio=4., qkv_bias=True,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1., upsampler='',
                 resi_connection='1conv', cpb_hidden=512, coords_table=None, **unused):
        depths = list(depths)
        heads = list(num_heads) if isinstance(num_heads, (list, tuple)) else [num_heads] * len(depths)
        nh = heads[0] if heads else 0
        hidden = int(embed_dim * mlp_ratio + 1e-6)
        unsupported = []
        if window_size != 8: unsupported.append(f'window_size={window_size} (8)')
        if patch_size != 1: unsupported.append(f'patch_size={patch_size} (1)')
        if not depths or any(not isinstance(d, int) or d < 1 for d in depths): unsupported.append(f'depths={depths}')
        if len(heads) != len(depths) or any(h != nh for h in heads): unsupported.append(f'num_heads={heads} (one count for every residual group)')
        elif not (isinstance(embed_dim, int) and 1 <= embed_dim <= 256 and isinstance(nh, int) and 1 <= nh <= 8 and embed_dim % nh == 0 and embed_dim // nh <= 32):
            unsupported.append(f'embed_dim={embed_dim}, num_heads={nh} (embed_dim <= 256, <= 8 heads of <= 32 channels, embed_dim % num_heads == 0)')
        if not 1 <= hidden <= 1024: unsupported.append(f'mlp_ratio={mlp_ratio} (int(embed_dim * mlp_ratio) = {hidden}; built: <= 1024)')
        if not qkv_bias: unsupported.append('qkv_bias=False')
        if ape: unsupported.append('ape=True (absolute_pos_embed)')
        if not patch_norm: unsupported.append('patch_norm=False')
        if img_range != 1: unsupported.append(f'img_range={img_range} (1)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if upsampler not in _TAILS:
            unsupported.append(f"upsampler={upsampler!r} (pixelshuffle, pixelshuffledirect, nearest+conv; pixelshuffle_aux is the compressed-SR form, pixelshuffle_hf the "
                               f"high-frequency one, '' the JPEG / denoising form)")
        elif upscale not in ((2, 4) if upsampler == 'nearest+conv' else (2, 3, 4)): unsupported.append(f'upscale={upscale} with {upsampler} ({"2, 4" if upsampler == "nearest+conv" else "2, 3, 4"})')
        if resi_connection not in ('1conv', '3conv'): unsupported.append(f'resi_connection={resi_connection!r}')
        if not isinstance(cpb_hidden, int) or cpb_hidden < 1: unsupported.append(f'cpb_hidden={cpb_hidden} (>= 1)')
        if coords_table is not None and tuple(np.shape(coords_table)) not in ((1, 15, 15, 2), (225, 2)):
            unsupported.append(f'coords_table of shape {tuple(np.shape(coords_table))} ((1, 15, 15, 2))')
        if unsupported:
            raise NotImplementedError('Swin2SR option(s) not built on the HIP path: ' + ', '.join(unsupported))
        EngineModule.__init__(self, swin2sr_shapes(in_chans, embed_dim, depths, nh, mlp_ratio, upscale, upsampler, resi_connection, window_size, cpb_hidden))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.num_heads, self.hidden, self.upscale = embed_dim, depths, nh, hidden, upscale
        self.upsampler, self.resi_connection, self.n_blocks, self.cpb_hidden = upsampler, resi_connection, sum(depths), cpb_hidden
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans
        # the coordinates cpb_mlp is evaluated on: a published checkpoint's buffer (authoritative when given), else the formula
        self.coords = relative_coords(8) if coords_table is None else np.asarray(coords_table, np.float64).reshape(225, 2)

    def _create_handle(self):
        h = C.c_void_p()
        depths = (C.c_int * len(self.depths))(*self.depths)
        mean = (C.c_float * 4)(*self.mean)
        L.check(L.lib.innfer_swin2sr_create(C.byref(h), self.in_nc, self.out_nc, self.nf, depths, len(self.depths), self.num_heads, self.hidden, _TAILS[self.upsampler],
                                            self.upscale, int(self.resi_connection == '3conv'), mean))
        return h

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: attn.qkv is put together from qkv.weight, q_bias and v_bias here (no scale); every other conv goes through SwinIR's relayout."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()
            f32 = lambda key: sd[key].detach().float().cpu().numpy()
            if base.endswith('attn.qkv'):
                a = base[:-len('qkv')]
                cache[base] = relayout_qkv(f32(base + '.weight'), f32(a + 'q_bias'), f32(a + 'v_bias'), self.nf, self.num_heads)
            else:
                w, b = EngineModule._conv_tensors(self, base, sd)
                cache[base] = relayout(base, w, b, self.nf, self.num_heads, self.hidden, self.in_nc, self.upscale, self.upsampler == 'pixelshuffledirect')
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def engine_tables(self, sd=None):
        """What _ensure_engine hands the library beside the convs, per block in forward order: (LayerNorm keys, dense bias tables [nH, 64, 64] float32, tau [nH] float32)."""
        sd = self.state_dict() if sd is None else sd
        f64 = lambda key: sd[key].detach().double().cpu().numpy()
        norms, tables, taus = ['patch_embed.norm'], [], []
        for i, depth in enumerate(self.depths):
            for j in range(depth):
                b = f'layers.{i}.residual_group.blocks.{j}.'
                norms += [b + 'norm1', b + 'norm2']
                tables.append(cpb_bias(f64(b + 'attn.cpb_mlp.0.weight'), f64(b + 'attn.cpb_mlp.0.bias'), f64(b + 'attn.cpb_mlp.2.weight'), self.coords))
                taus.append(attn_scale(f64(b + 'attn.logit_scale')))
        norms.append('norm')
        return norms, tables, taus

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        norms, tables, taus = self.engine_tables(sd)
        for blk, (t, tau) in enumerate(zip(tables, taus)):
            L.check(L.lib.innfer_net_set_attn_bias(self._handle, blk, t.ctypes.data))
            L.check(L.lib.innfer_net_set_attn_scale(self._handle, blk, tau.ctypes.data))
        for idx, key in enumerate(norms):
            g = np.ascontiguousarray(sd[key + '.weight'].detach().float().cpu().numpy())
            be = np.ascontiguousarray(sd[key + '.bias'].detach().float().cpu().numpy())
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, be.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'Swin2SR is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        for n in (H, W):
            if -n % 8 >= n:
                raise NotImplementedError(f'Swin2SR pads its input to multiples of 8 by reflection: a side of {n} pixels cannot be padded by {-n % 8} (the pad must be smaller than the side)')
