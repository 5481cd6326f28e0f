"""SwinIR shell (Liang et al. 2021: image restoration with a Swin transformer; the three super-resolution forms -- classical, lightweight, real-world).
The reference has no such architecture; constructor surface and state-dict keys are the published ones (KAIR / BasicSR swinir_arch.py), the graph is built inside
libinnfer_amd.so (csrc/net.hip, kind 5; csrc/win_attn.hip, csrc/layer_norm.hip, act 12 of csrc/conv3x3.hip).

    forward(x):   reflect-pad right / bottom to multiples of 8; f = conv_first(x - mean); f = conv_after_body(norm(RSTBs(patch_embed.norm(f)))) + f; tail; + mean; crop
    RSTB:         t = conv(blocks(t)) + t                ('1conv': one 3x3 conv; '3conv': 3x3 C -> C/4, LeakyReLU(0.2), 1x1, LeakyReLU(0.2), 3x3 C/4 -> C)
    block j:      t = t + proj(attn(norm1(t)));  t = t + fc2(GELU(fc1(norm2(t))))       (tokens = pixels; LayerNorm(C), eps 1e-5; exact GELU; shift 4 for odd j)
    attn:         8 x 8 windows of roll(u, (-shift, -shift)); per head softmax((q d^-0.5) k^T + B_h + M) v; M = -100 between regions of the rolled frame (shift only)
    tails:        pixelshuffle | pixelshuffledirect | nearest+conv

All weight re-layout happens at load, in fp32, before the engine's one fp16 rounding (`_conv_tensors`): C and the MLP's hidden size are padded to multiples of 64 with zero
weights and biases (pad channels stay zero everywhere: LayerNorm writes them as zeros, GELU(0) = LeakyReLU(0) = 0); every head gets one 32-channel group in each of q, k and
v (d real channels, then zeros), so attn.qkv's rows are permuted and attn.proj's input columns likewise; d^-0.5 goes into the q rows and their bias; `+ mean` into the last
conv's bias; `- mean` is the first conv's input map (the zero padding stays zero behind it).  The engine takes H x W and returns scale H x scale W: pad and crop are its own."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import swinir_shapes

RGB_MEAN = (0.4488, 0.4371, 0.4040)
_TAILS = {'pixelshuffle': 0, 'pixelshuffledirect': 1, 'nearest+conv': 2}


def relative_position_index(ws=8):
    """[ws^2, ws^2] long: (ri - rj + ws - 1) * (2 ws - 1) + (ci - cj + ws - 1) for tokens i = ws ri + ci, j = ws rj + cj -- the published buffer."""
    r = torch.arange(ws * ws) // ws
    c = torch.arange(ws * ws) % ws
    return (r[:, None] - r[None, :] + ws - 1) * (2 * ws - 1) + (c[:, None] - c[None, :] + ws - 1)


def dense_bias(table, ws=8):
    """relative_position_bias_table [(2 ws - 1)^2, nH] -> the dense [nH, ws^2 (query), ws^2 (key)] float32 table the attention kernel reads."""
    t = np.asarray(table, np.float32)
    return np.ascontiguousarray(t[relative_position_index(ws).numpy().reshape(-1)].reshape(ws * ws, ws * ws, -1).transpose(2, 0, 1))


def pad64(n):
    return -(-n // 64) * 64


def relayout(key, w, b, C_, nh, hidden, in_chans, scale, direct_tail):
    """The engine's weight and bias (float32 numpy) for the state-dict conv / Linear `key` of a SwinIR with embed_dim C_, nh heads, `hidden` MLP channels: [K_pad, C_in_pad, k, k]
    and [K_pad].  Pure index work and two folds (d^-0.5 into q, + mean into the last conv's bias), all in float32."""
    w = np.asarray(w, np.float32)
    b = np.zeros(w.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
    if w.ndim == 2:
        w = w[:, :, None, None]
    d, Cp, hp, c4, name = C_ // nh, pad64(C_), pad64(hidden), C_ // 4, key.split('.')

    def fit(w, b, rows, cols):               # zero-pad to [rows, cols, k, k] / [rows]
        wo = np.zeros((rows, cols) + w.shape[2:], np.float32)
        wo[:w.shape[0], :w.shape[1]] = w
        bo = np.zeros(rows, np.float32)
        bo[:b.shape[0]] = b
        return wo, bo
    if key.endswith('attn.qkv'):             # rows (q | k | v) x head x d -> group (which nh + h), 32 rows each; q rows and biases times d^-0.5
        rows = (3 * nh + 1) // 2 * 64
        wo, bo = np.zeros((rows, Cp, 1, 1), np.float32), np.zeros(rows, np.float32)
        sc = np.float32(d ** -0.5)
        for which in range(3):
            for h in range(nh):
                src = slice(which * C_ + h * d, which * C_ + (h + 1) * d)
                dst = slice((which * nh + h) * 32, (which * nh + h) * 32 + d)
                wo[dst, :C_] = w[src] * sc if which == 0 else w[src]
                bo[dst] = b[src] * sc if which == 0 else b[src]
        return wo, bo
    if key.endswith('attn.proj'):            # input columns head x d -> head x 32
        wo, bo = np.zeros((Cp, 32 * nh, 1, 1), np.float32), np.zeros(Cp, np.float32)
        for h in range(nh):
            wo[:C_, 32 * h:32 * h + d] = w[:, h * d:(h + 1) * d]
        bo[:C_] = b
        return wo, bo
    if key.endswith('mlp.fc1'):
        return fit(w, b, hp, Cp)
    if key.endswith('mlp.fc2'):
        return fit(w, b, Cp, hp)
    if key == 'conv_first':
        return fit(w, b, Cp, in_chans)
    if name[0] == 'layers' or name[0] == 'conv_after_body':          # resi_connection convs
        if name[-1] == '0' and name[-2] in ('conv', 'conv_after_body'):
            return fit(w, b, pad64(c4), Cp)
        if name[-1] == '2':
            return fit(w, b, pad64(c4), pad64(c4))
        if name[-1] == '4':
            return fit(w, b, Cp, pad64(c4))
        return fit(w, b, Cp, Cp)
    mean = np.asarray(RGB_MEAN if in_chans == 3 else (0.0,) * in_chans, np.float32)
    if key == 'conv_before_upsample.0':
        return fit(w, b, 64, Cp)
    if key == 'upsample.0' and direct_tail:
        wo, bo = fit(w, b, w.shape[0], Cp)
        return wo, bo + np.repeat(mean, scale * scale)
    if key == 'conv_last':
        return w, b + mean
    return w, b


class SwinIR(EngineModule):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1., upsampler='',
                 resi_connection='1conv', **unused):
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
        if qk_scale is not None: unsupported.append(f'qk_scale={qk_scale} (None: head_dim ** -0.5)')
        if ape: unsupported.append('ape=True (absolute_pos_embed)')
        if not patch_norm: unsupported.append('patch_norm=False')
        if img_range != 1: unsupported.append(f'img_range={img_range} (1)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if upsampler not in _TAILS: unsupported.append(f"upsampler={upsampler!r} (pixelshuffle, pixelshuffledirect, nearest+conv; '' is the denoising / JPEG form)")
        elif upscale not in ((2, 4) if upsampler == 'nearest+conv' else (2, 3, 4)): unsupported.append(f'upscale={upscale} with {upsampler} ({"2, 4" if upsampler == "nearest+conv" else "2, 3, 4"})')
        if resi_connection not in ('1conv', '3conv'): unsupported.append(f'resi_connection={resi_connection!r}')
        if unsupported:
            raise NotImplementedError('SwinIR option(s) not built on the HIP path: ' + ', '.join(unsupported))
        super().__init__(swinir_shapes(in_chans, embed_dim, depths, nh, mlp_ratio, upscale, upsampler, resi_connection, window_size))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.num_heads, self.hidden, self.upscale = embed_dim, depths, nh, hidden, upscale
        self.upsampler, self.resi_connection, self.n_blocks = upsampler, resi_connection, sum(depths)
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans

    def _io_sizes(self, H, W, s):
        """The engine pads to multiples of 8 and crops inside: it writes exactly the result."""
        return (H * s, W * s), (H * s, W * s)

    def _create_handle(self):
        h = C.c_void_p()
        depths = (C.c_int * len(self.depths))(*self.depths)
        mean = (C.c_float * 4)(*self.mean)
        L.check(L.lib.innfer_swinir_create(C.byref(h), self.in_nc, self.out_nc, self.nf, depths, len(self.depths), self.num_heads, self.hidden, _TAILS[self.upsampler],
                                           self.upscale, int(self.resi_connection == '3conv'), mean))
        return h

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: output channels 64 p .. 64 p + 63 of the re-laid-out weight (relayout); the tail's convs come whole."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()                    # (the slices of one conv are asked for in a row: one entry is enough)
            w, b = super()._conv_tensors(base, sd)
            cache[base] = relayout(base, w, b, self.nf, self.num_heads, self.hidden, self.in_nc, self.upscale, self.upsampler == 'pixelshuffledirect')
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        super()._ensure_engine()
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        f32 = lambda key: np.ascontiguousarray(sd[key].detach().float().cpu().numpy())
        norms = ['patch_embed.norm']
        blk = 0
        for i, depth in enumerate(self.depths):
            for j in range(depth):
                b = f'layers.{i}.residual_group.blocks.{j}.'
                norms += [b + 'norm1', b + 'norm2']
                table = dense_bias(f32(b + 'attn.relative_position_bias_table'))
                L.check(L.lib.innfer_net_set_attn_bias(self._handle, blk, table.ctypes.data))
                blk += 1
        norms.append('norm')
        for idx, key in enumerate(norms):
            g, be = f32(key + '.weight'), f32(key + '.bias')
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, be.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'SwinIR is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        for n in (H, W):
            if -n % 8 >= n:
                raise NotImplementedError(f'SwinIR pads its input to multiples of 8 by reflection: a side of {n} pixels cannot be padded by {-n % 8} (the pad must be smaller than the side)')

    def forward(self, x, outm=None, out=None):
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            raise self._fp16_only('a float32 input was given')
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'SwinIR has no outm ({outm!r})')
        if isinstance(x, torch.Tensor) and x.dim() == 4:
            self._check_size(x.shape[2], x.shape[3])
        return super().forward(x, None, out)

    def forward_u8(self, img, normalize=False, fp16=True, out=None):
        if not fp16:
            raise self._fp16_only('forward_u8(fp16=False) was asked for')
        if isinstance(img, torch.Tensor) and img.dim() in (3, 4):
            self._check_size(img.shape[-3], img.shape[-2])
        return super().forward_u8(img, normalize, True, out)

    def tile_batch_bytes(self, b, ps, dtype=torch.float16, device=None):
        if dtype == torch.float32:
            raise self._fp16_only('float32 tiles were asked for')
        return super().tile_batch_bytes(b, ps, dtype, device)
