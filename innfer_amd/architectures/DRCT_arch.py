"""DRCT shell (Hsu et al. 2024: "DRCT: Saving Image Super-Resolution away from Information Bottleneck"; DRCT, DRCT-L, Real-DRCT-GAN and their fine-tunes).
The reference has no such architecture; constructor surface and state-dict keys are the published ones (drct_arch.py, written down without the source at hand: that file
is the definition and a checkpoint's shapes are authoritative over the formulas here; keys.drct_shapes is the one table), the graph is built inside libinnfer_amd.so
(csrc/net.hip, kind 9; csrc/win_attn16_wide.hip, the holed form of csrc/layer_norm.hip, and HAT's win_attn16.hip / SwinIR's act 12).

With C = embed_dim, gc = 32, window 16, s = upscale:

    forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RDG_{R-1}(.. RDG_0(patch_embed.norm(f))))) + f;
                 conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop                              (mean, img_range 1: as SwinIR)
    RDG(x):      x_k = lrelu_0.2(adjust_k(swin_k(cat(x, x_1 .. x_{k-1}))))  k = 1 .. 4   (dim_k = C + 32 (k - 1) -> 32);
                 x_5 = adjust_5(swin_5(cat(x, x_1 .. x_4)))  (-> C, no activation);   return 0.2 x_5 + x          (adjust_k: a 1x1 conv with bias)
    swin_k(t):   SwinIR's block on dim_k channels: t = t + proj(attn(norm1(t)));  t = t + fc2(GELU(fc1(norm2(t))))
                 attn: 16 x 16 windows, shift 8 for k = 2, 4 (-100 between region labels of the rolled frame, as HAT's HAB); softmax(q d^-0.5 k^T + B_h + M) v,
                 B from relative_position_bias_table [961, nH_k]; nH_k heads of d = dim_k / nH_k: the published rule is num_heads - (dim_k % num_heads), the table decides

The engine never concatenates: one dense slab holds x in its own gx = ceil(C / 32) channel groups (pad channels zero) and x_k in group gx + k - 1.  A natural channel c of
cat(..) therefore sits at slab channel c (c < C) or 32 gx + (c - C): a HOLE [C, 32 gx) when C is no multiple of 32.  All re-layout happens at load, in FLOAT64, before
the one rounding to the float32 the engine takes (`_conv_tensors`, `slab_relayout`): the input columns of every norm, qkv, fc1 and adjust and the output rows of proj and fc2
go to slab order with zeros at the hole and the pads; qkv's rows and proj's columns to the head-padded order (head h of q / k / v in G = ceil(d / 32) groups of its own);
d^-0.5 into the q rows and their bias; the dense [nH][256][256] bias tables; `+ mean` into the last conv's bias."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import DRCT_GC, drct_head_rule, drct_shapes
from .SwinIR_arch import RGB_MEAN, SwinIR, pad64, relative_position_index

WS = 16


def slab_index(C_, dim):
    """Slab channel of every natural channel of cat(x, x_1, ..) with `dim` channels: c for c < C, else 32 ceil(C / 32) + (c - C)."""
    c = np.arange(dim)
    return np.where(c < C_, c, -(-C_ // 32) * 32 + (c - C_))


def dense_bias16(table):
    """relative_position_bias_table [961, nH] -> the dense [nH, 256, 256] float32 table the attention kernels read (a gather in float64: exact)."""
    t = np.asarray(table, np.float64)
    if t.ndim != 2 or t.shape[0] != (2 * WS - 1) ** 2:
        raise NotImplementedError(f'DRCT: a relative position bias table of shape {t.shape} ({(2 * WS - 1) ** 2} rows: window 16)')
    idx = relative_position_index(WS).numpy().reshape(-1)
    return np.ascontiguousarray(t[idx].reshape(WS * WS, WS * WS, -1).transpose(2, 0, 1).astype(np.float32))


def slab_relayout(kind, w, b, C_, k, nh, hidden):
    """The engine's weight [K_pad, C_in_pad, 1, 1] and bias [K_pad] (float32) of one Linear / 1x1 conv of block k (0 .. 4) of a dense group: `kind` is 'qkv', 'proj', 'fc1',
    'fc2' or 'adjust'.  Index work and one fold (d^-0.5 into q) in float64, then ONE rounding to float32."""
    w = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1])
    b = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    dim = C_ + DRCT_GC * k
    gx = -(-C_ // 32)
    cpk, d = 32 * (gx + k), dim // nh
    lp, hp, Gh = pad64(cpk), pad64(hidden), -(-d // 32)
    hg = nh * Gh
    pos = slab_index(C_, dim)
    hpos = (np.arange(dim) // d) * (32 * Gh) + np.arange(dim) % d          # natural head-major channel h d + j -> head-padded h 32 G + j
    if kind == 'qkv':
        rows = (3 * hg + 1) // 2 * 64
        wo, bo = np.zeros((rows, cpk)), np.zeros(rows)
        for which in range(3):
            sc = d ** -0.5 if which == 0 else 1.0
            dst = which * hg * 32 + hpos
            wo[dst[:, None], pos[None, :]] = w[which * dim:(which + 1) * dim] * sc
            bo[dst] = b[which * dim:(which + 1) * dim] * sc
    elif kind == 'proj':
        wo, bo = np.zeros((lp, 32 * hg)), np.zeros(lp)
        wo[pos[:, None], hpos[None, :]] = w
        bo[pos] = b
    elif kind == 'fc1':
        wo, bo = np.zeros((hp, cpk)), np.zeros(hp)
        wo[:hidden, pos] = w
        bo[:hidden] = b
    elif kind == 'fc2':
        wo, bo = np.zeros((lp, hp)), np.zeros(lp)
        wo[pos, :hidden] = w
        bo[pos] = b
    elif kind == 'adjust':
        rows = 64 if k < 4 else pad64(C_)          # (k < 4: 32 real rows, then 32 zero rows -- the launch clears the next group of the dense slab)
        wo, bo = np.zeros((rows, cpk)), np.zeros(rows)
        wo[:w.shape[0], pos] = w
        bo[:w.shape[0]] = b
    else:
        raise KeyError(kind)
    return wo.astype(np.float32)[:, :, None, None], bo.astype(np.float32)


class DRCT(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6), window_size=16, mlp_ratio=2.,
                 qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=2,
                 img_range=1., upsampler='', resi_connection='1conv', gc=32, block_heads=None, block_hidden=None, **unused):
        """depths: one entry per dense group (its value is not used: a group is five blocks).  block_heads / block_hidden: per block, 5 len(depths) ints read off a
        checkpoint (run._infer_drct); None: the published head rule on num_heads[0] and int(dim_k mlp_ratio)."""
        depths = list(depths)
        R = len(depths)
        heads = list(num_heads) if isinstance(num_heads, (list, tuple)) else [num_heads] * R
        nh0 = heads[0] if heads else 0
        unsupported = []
        ok_c = isinstance(embed_dim, int) and 1 <= embed_dim <= 256
        if window_size != WS: unsupported.append(f'window_size={window_size} ({WS})')
        if gc != DRCT_GC: unsupported.append(f'gc={gc} ({DRCT_GC})')
        if patch_size != 1: unsupported.append(f'patch_size={patch_size} (1)')
        if not ok_c: unsupported.append(f'embed_dim={embed_dim} (1 .. 256)')
        if not 1 <= R <= 64: unsupported.append(f'depths={depths} (1 .. 64 dense groups)')
        if ok_c and 1 <= R <= 64:
            if block_heads is None:
                if len(heads) != R or any(h != nh0 for h in heads) or not (isinstance(nh0, int) and nh0 >= 1):
                    unsupported.append(f'num_heads={heads} (one count for every dense group)')
                else:
                    block_heads = [drct_head_rule(embed_dim + DRCT_GC * k, nh0) for _ in range(R) for k in range(5)]
            if block_hidden is None:
                block_hidden = [int((embed_dim + DRCT_GC * k) * mlp_ratio + 1e-6) for _ in range(R) for k in range(5)]
            if block_heads is not None:
                block_heads, block_hidden = [int(v) for v in block_heads], [int(v) for v in block_hidden]
                if len(block_heads) != 5 * R or len(block_hidden) != 5 * R:
                    unsupported.append(f'{len(block_heads)} head counts and {len(block_hidden)} hidden sizes for {5 * R} blocks')
                else:
                    for blk, (nh, hid) in enumerate(zip(block_heads, block_hidden)):
                        dim = embed_dim + DRCT_GC * (blk % 5)
                        if not 1 <= nh <= 8 or dim % nh or dim // nh > 128:
                            unsupported.append(f'block {blk}: {nh} heads on {dim} channels (<= 8 heads of <= 128 channels, dim % heads == 0)')
                        if not 1 <= hid <= 1024:
                            unsupported.append(f'block {blk}: an MLP of {hid} hidden channels (<= 1024)')
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
            raise NotImplementedError('DRCT option(s) not built on the HIP path: ' + ', '.join(unsupported))
        EngineModule.__init__(self, drct_shapes(in_chans, embed_dim, R, nh0, mlp_ratio, upscale, block_heads, block_hidden))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.depths, self.n_groups, self.upscale = embed_dim, depths, R, upscale
        self.block_heads, self.block_hidden = block_heads, block_hidden
        # the published head rule: recorded, never assumed
        self.heads_follow_rule = isinstance(nh0, int) and nh0 >= 1 and block_heads == [drct_head_rule(embed_dim + DRCT_GC * k, nh0) for _ in range(R) for k in range(5)]
        self.num_heads, self.hidden = block_heads[0], max(block_hidden)
        self.upsampler, self.resi_connection, self.n_blocks = upsampler, resi_connection, 5 * R
        self.mean = RGB_MEAN if in_chans == 3 else (0.0,) * in_chans

    def _create_handle(self):
        h = C.c_void_p()
        n = len(self.block_heads)
        heads, hidden = (C.c_int * n)(*self.block_heads), (C.c_int * n)(*self.block_hidden)
        mean = (C.c_float * 4)(*self.mean)
        L.check(L.lib.innfer_drct_create(C.byref(h), self.in_nc, self.out_nc, self.nf, self.n_groups, heads, hidden, self.upscale, mean))
        return h

    def launches(self, padded):
        """Launches of one forward: 2 S1 + 2 + sum over blocks (3 + SQ + 2 S + SH + A) + T + 2 [padded]."""
        S1, gx = pad64(self.nf) // 64, -(-self.nf // 32)
        n = 2 * S1 + 2 + (4 if self.upscale == 3 else 2 + {2: 1, 4: 2}[self.upscale]) + (2 if padded else 0)
        for blk, (nh, hid) in enumerate(zip(self.block_heads, self.block_hidden)):
            k = blk % 5
            d = (self.nf + DRCT_GC * k) // nh
            n += 3 + (3 * nh * -(-d // 32) + 1) // 2 + 2 * (pad64(32 * (gx + k)) // 64) + pad64(hid) // 64 + (1 if k < 4 else S1)
        return n

    def _block_of(self, base):
        """(group, k 0 .. 4, kind) of the engine key `layers.<g>.swin<k>.<...>` / `layers.<g>.adjust<k>`, or None."""
        name = base.split('.')
        if name[0] != 'layers' or len(name) < 3:
            return None
        if name[2].startswith('adjust'):
            return int(name[1]), int(name[2][6:]) - 1, 'adjust'
        kind = {'attn.qkv': 'qkv', 'attn.proj': 'proj', 'mlp.fc1': 'fc1', 'mlp.fc2': 'fc2'}['.'.join(name[3:])]
        return int(name[1]), int(name[2][4:]) - 1, kind

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: output channels 64 p .. 64 p + 63 of the re-laid-out weight; the tail's convs come whole."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()                    # (the slices of one conv are asked for in a row: one entry is enough)
            w, b = EngineModule._conv_tensors(self, base, sd)
            blk = self._block_of(base)
            Cp = pad64(self.nf)
            if blk is not None:
                g, kk, kind = blk
                cache[base] = slab_relayout(kind, w, b, self.nf, kk, self.block_heads[5 * g + kk], self.block_hidden[5 * g + kk])
            elif base in ('conv_first', 'conv_after_body', 'conv_before_upsample.0'):
                rows, cols = (64 if base.startswith('conv_before') else Cp), (self.in_nc if base == 'conv_first' else Cp)
                wo, bo = np.zeros((rows, cols, 3, 3), np.float32), np.zeros(rows, np.float32)
                wo[:w.shape[0], :w.shape[1]] = w
                bo[:b.shape[0]] = b
                cache[base] = (wo, bo)
            elif base == 'conv_last':
                cache[base] = (w, (np.asarray(b, np.float64) + np.asarray(self.mean, np.float64)).astype(np.float32))
            else:
                cache[base] = (w, b)
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def engine_tables(self, sd=None):
        """What _ensure_engine hands the library beside the convs, in forward order: LayerNorm (gamma, beta) pairs in SLAB order and the dense bias tables."""
        sd = self.state_dict() if sd is None else sd
        f64 = lambda key: sd[key].detach().double().cpu().numpy()
        Cp, gx = pad64(self.nf), -(-self.nf // 32)

        def norm(key, dim, width):
            g, b = np.zeros(width, np.float32), np.zeros(width, np.float32)
            pos = slab_index(self.nf, dim)
            g[pos], b[pos] = f64(key + '.weight'), f64(key + '.bias')
            return g, b
        norms, tables = [norm('patch_embed.norm', self.nf, Cp)], []
        for i in range(self.n_groups):
            for k in range(5):
                b = f'layers.{i}.swin{k + 1}.'
                dim, lp = self.nf + DRCT_GC * k, pad64(32 * (gx + k))
                norms += [norm(b + 'norm1', dim, lp), norm(b + 'norm2', dim, lp)]
                t = dense_bias16(f64(b + 'attn.relative_position_bias_table'))
                if t.shape[0] != self.block_heads[5 * i + k]:
                    raise RuntimeError(f'DRCT: {b}attn.relative_position_bias_table has {t.shape[0]} heads, the shell was built for {self.block_heads[5 * i + k]}')
                tables.append(t)
        norms.append(norm('norm', self.nf, Cp))
        return norms, tables

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        norms, tables = self.engine_tables()
        for idx, t in enumerate(tables):
            L.check(L.lib.innfer_net_set_attn_bias(self._handle, idx, t.ctypes.data))
        for idx, (g, b) in enumerate(norms):
            L.check(L.lib.innfer_net_set_layer_norm(self._handle, idx, g.ctypes.data, b.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'DRCT is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        for n in (H, W):
            if -n % 16 >= n:
                raise NotImplementedError(f'DRCT pads its input to multiples of 16 by reflection: a side of {n} pixels cannot be padded by {-n % 16} (the pad must be smaller than the side)')

    def forward(self, x, outm=None, out=None):
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'DRCT has no outm ({outm!r})')
        return super().forward(x, None, out)
