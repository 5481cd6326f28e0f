"""SRFormer shell (Zhou et al. 2023: "SRFormer: Permuted Self-Attention for Single Image Super-Resolution"; the light, classical and real-world forms).
The reference has no such architecture.  Written down without the published source at hand: the formulas of include/innfer_amd.h are the definition, a checkpoint's shapes
are authoritative for sizes.  The graph is built inside libinnfer_amd.so (csrc/net.hip, kind 10; csrc/win_attn_perm.hip, csrc/dwconv5.hip).  SwinIR's skeleton
(SwinIR_arch.py: pad, mean, conv_first, patch_embed.norm, RSTB = conv(blocks(t)) + t, norm, conv_after_body + f, tails, crop) on windows of ws = 16 | 22 | 24 around another block:

    block j:   t = t + proj(PSA(norm1(t)));  t = t + fc2(h + GELU(dw5x5(h))),  h = GELU(fc1(norm2(t)))         (shift ws / 2 for odd j)
    PSA:       ws^2 queries, (ws / 2)^2 keys per window: a key token takes the C / 4 channels of kv's k (v) output at the four pixels of a 2 x 2 patch, s = 0 .. 3 major
    bias:      B[h][(r, c)][(py, px)] = table[(r // 2 - py + pw - 1)(2 pw - 1) + (c // 2 - px + pw - 1)][h], pw = ws / 2

Load-time work, in float64 before the engine's one fp16 rounding (`_conv_tensors` hands float32 over): d^-0.5 into attn.q's rows and bias, head h's d rows at 32 h of the
q slab; attn.kv's k rows, zero-padded to whole 32-groups, then its v rows; `+ mean` into the last conv's bias; every other tensor through SwinIR's relayout (index work).
The bias table goes over COMPACT ([nH][(2 pw - 1)^2]): the attention kernel gathers from it."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import srformer_shapes
from .SwinIR_arch import _TAILS, RGB_MEAN, SwinIR, pad64, relayout

WINDOWS = (16, 22, 24)


def aligned_relative_position_index(ws):
    """[ws^2, (ws / 2)^2] long: (r // 2 - py + pw - 1)(2 pw - 1) + (c // 2 - px + pw - 1) for query (r, c) and key (py, px) -- the published buffer."""
    pw = ws // 2
    r, c = torch.arange(ws * ws) // ws // 2, torch.arange(ws * ws) % ws // 2
    py, px = torch.arange(pw * pw) // pw, torch.arange(pw * pw) % pw
    return (r[:, None] - py[None, :] + pw - 1) * (2 * pw - 1) + (c[:, None] - px[None, :] + pw - 1)


def relayout_q(w, b, C_, nh):
    """attn.q for the engine: head h's d rows at 32 h (zero pads), times d^-0.5 in float64; ceil(nh / 2) slices of 64 rows."""
    d, rows = C_ // nh, (nh + 1) // 2 * 64
    w, b = np.asarray(w, np.float64) * d ** -0.5, np.asarray(b, np.float64) * d ** -0.5
    wo, bo = np.zeros((rows, pad64(C_), 1, 1)), np.zeros(rows)
    for h in range(nh):
        wo[32 * h:32 * h + d, :C_, 0, 0] = w[h * d:(h + 1) * d]
        bo[32 * h:32 * h + d] = b[h * d:(h + 1) * d]
    return wo.astype(np.float32), bo.astype(np.float32)


def relayout_kv(w, b, C_):
    """attn.kv for the engine: k's C / 4 rows in natural order in ceil(C / 128) groups of 32 (zero pads), then v's likewise."""
    c4 = C_ // 4
    kg = -(-c4 // 32)
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    wo, bo = np.zeros((kg * 64, pad64(C_), 1, 1)), np.zeros(kg * 64)
    for which in range(2):
        wo[32 * kg * which:32 * kg * which + c4, :C_, 0, 0] = w[which * c4:(which + 1) * c4]
        bo[32 * kg * which:32 * kg * which + c4] = b[which * c4:(which + 1) * c4]
    return wo.astype(np.float32), bo.astype(np.float32)


class SRFormer(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6), window_size=22, mlp_ratio=2., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1., upsampler='',
                 resi_connection='1conv', **unused):
        depths = list(depths)
        heads = list(num_heads) if isinstance(num_heads, (list, tuple)) else [num_heads] * len(depths)
        nh = heads[0] if heads else 0
        hidden = int(embed_dim * mlp_ratio + 1e-6)
        unsupported = []
        if window_size not in WINDOWS: unsupported.append(f'window_size={window_size} (16, 22, 24)')
        if patch_size != 1: unsupported.append(f'patch_size={patch_size} (1)')
        if not depths or any(not isinstance(d, int) or d < 1 for d in depths): unsupported.append(f'depths={depths}')
        if len(heads) != len(depths) or any(h != nh for h in heads): unsupported.append(f'num_heads={heads} (one count for every residual group)')
        elif not (isinstance(embed_dim, int) and 1 <= embed_dim <= 256 and embed_dim % 4 == 0 and isinstance(nh, int) and 1 <= nh <= 8 and embed_dim % nh == 0 and embed_dim // nh <= 32):
            unsupported.append(f'embed_dim={embed_dim}, num_heads={nh} (embed_dim <= 256 and a multiple of 4, <= 8 heads of <= 32 channels, embed_dim % num_heads == 0)')
        if not 1 <= hidden <= 1024: unsupported.append(f'mlp_ratio={mlp_ratio} (int(embed_dim * mlp_ratio) = {hidden}; built: hidden <= 1024)')
        if not qkv_bias: unsupported.append('qkv_bias=False')
        if qk_scale is not None: unsupported.append(f'qk_scale={qk_scale} (None: head_dim ** -0.5)')
        if ape: unsupported.append('ape=True (absolute_pos_embed)')
        if not patch_norm: unsupported.append('patch_norm=False')
        if img_range != 1: unsupported.append(f'img_range={img_range} (1)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if upsampler not in _TAILS: unsupported.append(f"upsampler={upsampler!r} (pixelshuffle, pixelshuffledirect, nearest+conv; '' is the denoising / JPEG form)")
        elif upscale not in ((2, 4) if upsampler == 'nearest+conv' else (2, 3, 4)): unsupported.append(f'upscale={upscale} with {upsampler} ({"2, 4" if upsampler == "nearest+conv" else "2, 3, 4"})')
        if resi_connection not in ('1conv', '3conv'): unsupported.append(f'resi_connection={resi_connection!r}')
        if unsupported:
            raise NotImplementedError('SRFormer option(s) not built on the HIP path: ' + ', '.join(unsupported))
        EngineModule.__init__(self, srformer_shapes(in_chans, embed_dim, depths, nh, mlp_ratio, upscale, upsampler, resi_connection, window_size))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.num_heads, self.hidden, self.upscale = embed_dim, depths, nh, hidden, upscale
        self.upsampler, self.resi_connection, self.n_blocks, self.window_size = upsampler, resi_connection, sum(depths), window_size
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans

    def _create_handle(self):
        h = C.c_void_p()
        depths = (C.c_int * len(self.depths))(*self.depths)
        mean = (C.c_float * 4)(*self.mean)
        L.check(L.lib.innfer_srformer_create(C.byref(h), self.in_nc, self.out_nc, self.nf, depths, len(self.depths), self.num_heads, self.hidden, self.window_size,
                                             _TAILS[self.upsampler], self.upscale, int(self.resi_connection == '3conv'), mean))
        return h

    def relayout(self, base, w, b):
        """The engine's float32 (weight, bias) of the state-dict conv / Linear `base`; w, b: float64 numpy (b may be None)."""
        direct = self.upsampler == 'pixelshuffledirect'
        if base.endswith('attn.q'):
            return relayout_q(w, b, self.nf, self.num_heads)
        if base.endswith('attn.kv'):
            return relayout_kv(w, b, self.nf)
        mean = np.asarray(self.mean, np.float32).astype(np.float64)
        if base == 'conv_last':                                                # + mean in float64
            return w.astype(np.float32), (b + mean).astype(np.float32)
        if base == 'upsample.0' and direct:                                    # likewise, once per phase; input channels padded with zeros
            wo = np.zeros((w.shape[0], pad64(self.nf)) + w.shape[2:], np.float32)
            wo[:, :self.nf] = w
            return wo, (b + np.repeat(mean, self.upscale ** 2)).astype(np.float32)
        return relayout(base, w, b, self.nf, self.num_heads, self.hidden, self.in_nc, self.upscale, direct)

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: output channels 64 p .. 64 p + 63 of the re-laid-out weight; the tail's convs come whole."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()
            f64 = lambda key: sd[key].detach().double().cpu().numpy()
            cache[base] = self.relayout(base, f64(base + '.weight'), f64(base + '.bias'))
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def engine_tables(self, sd=None):
        """What _ensure_engine hands the library beside the convs, per block in forward order: (LayerNorm keys, compact bias tables [nH, (ws - 1)^2] float32, depthwise
        taps [hidden, 25] float32, depthwise biases [hidden] float32)."""
        sd = self.state_dict() if sd is None else sd
        f32 = lambda key: np.ascontiguousarray(sd[key].detach().float().cpu().numpy())
        norms, tables, taps, biases = ['patch_embed.norm'], [], [], []
        for i, depth in enumerate(self.depths):
            for j in range(depth):
                b = f'layers.{i}.residual_group.blocks.{j}.'
                norms += [b + 'norm1', b + 'norm2']
                tables.append(np.ascontiguousarray(f32(b + 'attn.relative_position_bias_table').T))
                taps.append(np.ascontiguousarray(f32(b + 'mlp.dwconv.depthwise_conv.0.weight').reshape(self.hidden, 25)))
                biases.append(f32(b + 'mlp.dwconv.depthwise_conv.0.bias'))
        norms.append('norm')
        return norms, tables, taps, biases

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        norms, tables, taps, biases = self.engine_tables(sd)
        for blk, (t, w, b) in enumerate(zip(tables, taps, biases)):
            L.check(L.lib.innfer_net_set_attn_bias(self._handle, blk, t.ctypes.data))
            L.check(L.lib.innfer_net_set_dwconv5(self._handle, blk, w.ctypes.data, b.ctypes.data))
        for idx, key in enumerate(norms):
            g = np.ascontiguousarray(sd[key + '.weight'].detach().float().cpu().numpy())
            be = np.ascontiguousarray(sd[key + '.bias'].detach().float().cpu().numpy())
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, be.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'SRFormer is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    def _check_size(self, H, W):
        ws = self.window_size
        for n in (H, W):
            if -n % ws >= n:
                raise NotImplementedError(f'SRFormer pads its input to multiples of {ws} by reflection: a side of {n} pixels cannot be padded by {-n % ws} (the pad must be smaller than the side)')
