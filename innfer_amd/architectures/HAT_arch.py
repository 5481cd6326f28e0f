"""HAT shell (Chen et al. 2023: "Activating More Pixels in Image Super-Resolution Transformer"; HAT-S, HAT, HAT-L, Real_HAT_GAN_SRx4 and their fine-tunes).
The reference has no such architecture; constructor surface and state-dict keys are the published ones (hat_arch.py), the graph is built inside libinnfer_amd.so
(csrc/net.hip, kind 6; csrc/win_attn16.hip, csrc/chan_attn.hip, act 13 of csrc/conv3x3.hip, and SwinIR's layer_norm.hip / act 12).

With C = embed_dim, nH heads of d = C / nH, window ws = 16, ows = ws + int(0.5 ws) = 24, s = upscale:

    forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RHAGs(patch_embed.norm(f)))) + f;
                 conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop                              (mean, img_range 1: as SwinIR)
    RHAG i:      t = conv(OCAB(HAB_{n-1}(... HAB_0(t)))) + t
    HAB j:       u = norm1(t);  t = t + proj(attn(u)) + conv_scale * CAB(u);  t = t + fc2(GELU(fc1(norm2(t))))
                 attn: SwinIR's window attention with ws 16, shift 8 for odd j; mask -100 between region labels of the rolled frame (rows / columns split at Hp - 16 and
                 Hp - 8), computed per input size; bias from table [(2 ws - 1)^2, nH]
    CAB(u):      z = conv3x3(C -> C / compress_ratio) -> exact GELU -> conv3x3(C / compress_ratio -> C);  y = sigmoid(W2 relu(W1 mean_pixels(z) + b1) + b2);
                 CAB = z * y[channel]        -- the mean runs over the whole padded Hp x Wp grid of ONE sample
    OCAB:        u = norm1(t); q, k, v = qkv(u) (channel order [3][nH][d]); queries: the 16 x 16 windows, q * d^-0.5; keys / values of window (wy, wx): the 24 x 24
                 pixels from (16 wy - 4, 16 wx - 4) (nn.Unfold(24, stride 16, padding 4) applied AFTER the Linear): a position outside the padded grid has k = v = 0 --
                 its score is the bias alone and it DOES take part in the softmax; softmax(q k^T + B) v; no shift, no mask; t = t + proj(.);
                 t = t + fc2(GELU(fc1(norm2(t))));  B[i][j] = table[idx[i][j]][h], table [(ws + ows - 1)^2, nH]

`conv_scale` is a constructor float and is NOT in the state dict (every published model uses 0.01).  Published checkpoints carry two top-level buffers,
relative_position_index_SA [256, 256] and relative_position_index_OCA [256, 576]; when present they are what the dense bias tables are built from (run._infer_hat hands
them over as `rpi_sa` / `rpi_oca` and drops them from the state dict), otherwise the formulas below.  The OCA formula is written from memory of the published code: the
stored buffer is the safeguard.  Weight re-layout is SwinIR's (SwinIR_arch.relayout); the conv block's 3x3 convs are padded to 64 middle channels."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import hat_shapes
from .SwinIR_arch import RGB_MEAN, SwinIR, pad64, relative_position_index, relayout

WS, OWS = 16, 24


def relative_position_index_oca(ws=WS, ows=OWS):
    """[ws^2, ows^2] long: (ry_j - ry_i + ws - ows + 1) (ws + ows - 1) + (rx_j - rx_i + ws - ows + 1) for query i at (ry_i, rx_i) of its ws x ws window and key j at
    (ry_j, rx_j) of its ows x ows window.  Entries may be negative: they index the table from its end, as torch indexing does."""
    qy, qx = torch.arange(ws * ws) // ws, torch.arange(ws * ws) % ws
    ky, kx = torch.arange(ows * ows) // ows, torch.arange(ows * ows) % ows
    off = ws - ows + 1
    return (ky[None, :] - qy[:, None] + off) * (ws + ows - 1) + (kx[None, :] - qx[:, None] + off)


def dense_bias_indexed(table, index):
    """relative_position_bias_table [rows, nH] and an index [queries, keys] -> the dense [nH, queries, keys] float32 table the attention kernel reads.  Negative entries
    index from the end of the table (the torch rule); entries outside [-rows, rows) are refused."""
    t = np.asarray(table, np.float32)
    idx = np.asarray(index, np.int64)
    if idx.ndim != 2 or idx.min() < -t.shape[0] or idx.max() >= t.shape[0]:
        raise NotImplementedError(f'HAT: a relative position index of shape {tuple(idx.shape)} with entries {int(idx.min())} .. {int(idx.max())} does not address a table of {t.shape[0]} rows')
    return np.ascontiguousarray(t[idx.reshape(-1)].reshape(idx.shape[0], idx.shape[1], -1).transpose(2, 0, 1))


class HAT(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7, compress_ratio=3, squeeze_factor=30,
                 conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, ape=False,
                 patch_norm=True, use_checkpoint=False, upscale=2, img_range=1., upsampler='', resi_connection='1conv', rpi_sa=None, rpi_oca=None, **unused):
        depths = list(depths)
        heads = list(num_heads) if isinstance(num_heads, (list, tuple)) else [num_heads] * len(depths)
        nh = heads[0] if heads else 0
        hidden = int(embed_dim * mlp_ratio + 1e-6)
        unsupported = []
        if window_size != WS: unsupported.append(f'window_size={window_size} ({WS})')
        elif window_size + int(overlap_ratio * window_size) != OWS: unsupported.append(f'overlap_ratio={overlap_ratio} (0.5: an overlapping window of {OWS})')
        if patch_size != 1: unsupported.append(f'patch_size={patch_size} (1)')
        if not depths or any(not isinstance(d, int) or d < 1 for d in depths): unsupported.append(f'depths={depths}')
        if len(heads) != len(depths) or any(h != nh for h in heads): unsupported.append(f'num_heads={heads} (one count for every residual group)')
        elif not (isinstance(embed_dim, int) and 1 <= embed_dim <= 256 and isinstance(nh, int) and 1 <= nh <= 8 and embed_dim % nh == 0 and embed_dim // nh <= 32):
            unsupported.append(f'embed_dim={embed_dim}, num_heads={nh} (embed_dim <= 256, <= 8 heads of <= 32 channels, embed_dim % num_heads == 0)')
        if not 1 <= hidden <= 1024: unsupported.append(f'mlp_ratio={mlp_ratio} (int(embed_dim * mlp_ratio) = {hidden}; built: <= 1024)')
        ok_c = isinstance(embed_dim, int) and embed_dim >= 1
        if not (ok_c and isinstance(compress_ratio, int) and compress_ratio >= 1 and 1 <= embed_dim // compress_ratio <= 64):
            unsupported.append(f'compress_ratio={compress_ratio} (embed_dim // compress_ratio in 1 .. 64)')
        if not (ok_c and isinstance(squeeze_factor, int) and squeeze_factor >= 1 and 1 <= embed_dim // squeeze_factor <= 64):
            unsupported.append(f'squeeze_factor={squeeze_factor} (embed_dim // squeeze_factor in 1 .. 64)')
        if not qkv_bias: unsupported.append('qkv_bias=False')
        if qk_scale is not None: unsupported.append(f'qk_scale={qk_scale} (None: head_dim ** -0.5)')
        if ape: unsupported.append('ape=True (absolute_pos_embed)')
        if not patch_norm: unsupported.append('patch_norm=False')
        if img_range != 1: unsupported.append(f'img_range={img_range} (1)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if upsampler != 'pixelshuffle': unsupported.append(f"upsampler={upsampler!r} (pixelshuffle)")
        elif upscale not in (2, 3, 4): unsupported.append(f'upscale={upscale} (2, 3, 4)')
        if resi_connection != '1conv': unsupported.append(f'resi_connection={resi_connection!r} (1conv)')
        if unsupported:
            raise NotImplementedError('HAT option(s) not built on the HIP path: ' + ', '.join(unsupported))
        EngineModule.__init__(self, hat_shapes(in_chans, embed_dim, depths, nh, mlp_ratio, upscale, compress_ratio, squeeze_factor))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.num_heads, self.hidden, self.upscale = embed_dim, depths, nh, hidden, upscale
        self.upsampler, self.resi_connection, self.n_blocks = upsampler, resi_connection, sum(depths)
        self.compress_ch, self.squeeze_ch, self.conv_scale = embed_dim // compress_ratio, embed_dim // squeeze_factor, float(conv_scale)
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans
        # the index buffers of a published checkpoint (authoritative when given), else the formulas
        self.rpi_sa = np.asarray(relative_position_index(WS) if rpi_sa is None else rpi_sa, np.int64)
        self.rpi_oca = np.asarray(relative_position_index_oca() if rpi_oca is None else rpi_oca, np.int64)
        if self.rpi_sa.shape != (WS * WS, WS * WS) or self.rpi_oca.shape != (WS * WS, OWS * OWS):
            raise NotImplementedError(f'HAT: relative position indices of shape {self.rpi_sa.shape} / {self.rpi_oca.shape} ({(WS * WS, WS * WS)} / {(WS * WS, OWS * OWS)})')
        for idx, rows in ((self.rpi_sa, (2 * WS - 1) ** 2), (self.rpi_oca, (WS + OWS - 1) ** 2)):
            dense_bias_indexed(np.zeros((rows, 1), np.float32), idx)         # (refuses entries outside [-rows, rows) here, before the GPU is touched)

    def _create_handle(self):
        h = C.c_void_p()
        depths = (C.c_int * len(self.depths))(*self.depths)
        mean = (C.c_float * 4)(*self.mean)
        L.check(L.lib.innfer_hat_create(C.byref(h), self.in_nc, self.out_nc, self.nf, depths, len(self.depths), self.num_heads, self.hidden, self.compress_ch,
                                        self.squeeze_ch, self.upscale, mean))
        return h

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`; the conv block's convs are padded to 64 middle channels here, every other conv goes through SwinIR's relayout."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()
            w, b = EngineModule._conv_tensors(self, base, sd)
            if base.endswith('conv_block.cab.0') or base.endswith('conv_block.cab.2'):
                first = base.endswith('.0')
                rows, cols = (64, pad64(self.nf)) if first else (pad64(self.nf), 64)
                wo, bo = np.zeros((rows, cols, 3, 3), np.float32), np.zeros(rows, np.float32)
                wo[:w.shape[0], :w.shape[1]] = w
                bo[:b.shape[0]] = b
                cache[base] = (wo, bo)
            else:
                cache[base] = relayout(base, w, b, self.nf, self.num_heads, self.hidden, self.in_nc, self.upscale, False)
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def engine_tables(self, sd=None):
        """What _ensure_engine hands the library beside the convs, in forward order: (LayerNorm keys, dense bias tables, channel-attention tensors per HAB)."""
        sd = self.state_dict() if sd is None else sd
        f32 = lambda key: np.ascontiguousarray(sd[key].detach().float().cpu().numpy())
        norms, tables, cas = ['patch_embed.norm'], [], []
        for i, depth in enumerate(self.depths):
            g = f'layers.{i}.residual_group.'
            for j in range(depth):
                b = g + f'blocks.{j}.'
                norms += [b + 'norm1', b + 'norm2']
                tables.append(dense_bias_indexed(f32(b + 'attn.relative_position_bias_table'), self.rpi_sa))
                a = b + 'conv_block.cab.3.attention.'
                cas.append(tuple(np.ascontiguousarray(f32(a + k).reshape(f32(a + k).shape[0], -1)) for k in ('1.weight', '1.bias', '3.weight', '3.bias')))
            norms += [g + 'overlap_attn.norm1', g + 'overlap_attn.norm2']
            tables.append(dense_bias_indexed(f32(g + 'overlap_attn.relative_position_bias_table'), self.rpi_oca))
        norms.append('norm')
        return norms, tables, cas

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        norms, tables, cas = self.engine_tables(sd)
        for idx, t in enumerate(tables):
            L.check(L.lib.innfer_net_set_attn_bias(self._handle, idx, t.ctypes.data))
        for blk, (w1, b1, w2, b2) in enumerate(cas):
            L.check(L.lib.innfer_net_set_chan_attn(self._handle, blk, w1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data))
        for idx, key in enumerate(norms):
            g = np.ascontiguousarray(sd[key + '.weight'].detach().float().cpu().numpy())
            be = np.ascontiguousarray(sd[key + '.bias'].detach().float().cpu().numpy())
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, be.ctypes.data))
        L.check(L.lib.innfer_net_set_conv_scale(self._handle, self.conv_scale))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'HAT is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        for n in (H, W):
            if -n % 16 >= n:
                raise NotImplementedError(f'HAT pads its input to multiples of 16 by reflection: a side of {n} pixels cannot be padded by {-n % 16} (the pad must be smaller than the side)')

    def forward(self, x, outm=None, out=None):
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'HAT has no outm ({outm!r})')
        return super().forward(x, None, out)
