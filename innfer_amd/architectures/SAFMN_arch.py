"""SAFMN shell (Sun et al. 2023: "Spatially-Adaptive Feature Modulation for Efficient Image Super-Resolution"; SAFMN and SAFMN-L).
The reference has no such architecture; constructor names and state-dict keys are the published ones (safmn_arch.py, BasicSR), include/innfer_amd.h carries the definition,
the graph is built inside libinnfer_amd.so (csrc/net.hip, kind 11; csrc/safm.hip, csrc/layer_norm.hip, acts 12 / 13 of csrc/conv3x3.hip).

    forward(x):  f = to_feat(x); f = feats(f) + f; y = PixelShuffle(s)(to_img.0(f))
    AttBlock:    t = t + safm(norm1(t));  t = t + ccm.2(GELU(ccm.0(norm2(t))))              (LayerNorm over a pixel's channels, eps 1e-6; exact GELU)
    safm(u):     four levels of dim / 4 channels: max-pool to (h >> i, w >> i), depthwise 3 x 3, nearest back; GELU(aggr(cat)) * u -- ONE launch

Load-time work is index work in float32: dim and hidden are padded to multiples of 64 with zero weights and biases (pad channels stay zero everywhere: LayerNorm and the
feature modulation write them as zeros, GELU(0) = 0), the four mfr convs go over as one [dim][9] array.  No size is padded: the engine takes any H x W >= 8 x 8."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import safmn_shapes
from .SwinIR_arch import SwinIR, pad64


class SAFMN(SwinIR):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, dim=36, n_blocks=8, ffn_scale=2.0, upscaling_factor=4, in_chans=3, **unused):
        hidden = int(dim * ffn_scale + 1e-6) if isinstance(dim, int) else 0
        unsupported = []
        if not (isinstance(dim, int) and 8 <= dim <= 256 and dim % 4 == 0): unsupported.append(f'dim={dim} (a multiple of 4 in 8 .. 256)')
        if not (isinstance(n_blocks, int) and 1 <= n_blocks <= 256): unsupported.append(f'n_blocks={n_blocks}')
        if not 1 <= hidden <= 1024: unsupported.append(f'ffn_scale={ffn_scale} (int(dim * ffn_scale) = {hidden}; built: 1 .. 1024)')
        if upscaling_factor not in (1, 2, 3, 4): unsupported.append(f'upscaling_factor={upscaling_factor} (1 .. 4)')
        if not isinstance(in_chans, int) or not 1 <= in_chans <= 4: unsupported.append(f'in_chans={in_chans} (1..4)')
        if unsupported:
            raise NotImplementedError('SAFMN option(s) not built on the HIP path: ' + ', '.join(unsupported))
        EngineModule.__init__(self, safmn_shapes(dim, n_blocks, ffn_scale, upscaling_factor, in_chans))
        self.in_nc = self.out_nc = in_chans
        self.nf, self.n_blocks, self.hidden, self.upscale = dim, n_blocks, hidden, upscaling_factor

    def _create_handle(self):
        h = C.c_void_p()
        L.check(L.lib.innfer_safmn_create(C.byref(h), self.in_nc, self.out_nc, self.nf, self.n_blocks, self.hidden, self.upscale))
        return h

    def _conv_tensors(self, k, sd):
        """Engine key `<state-dict key>#<p>`: output channels 64 p .. 64 p + 63 of the conv padded with zeros to whole 64s; safm.aggr and to_img.0 come whole (to_img.0
        with its input channels padded)."""
        base, _, p = k.partition('#')
        cache = self.__dict__.setdefault('_relayout_cache', {})
        if base not in cache:
            cache.clear()                    # (the slices of one conv are asked for in a row: one entry is enough)
            w, b = EngineModule._conv_tensors(self, base, sd)
            if not base.endswith('safm.aggr'):
                rows = w.shape[0] if base == 'to_img.0' else pad64(w.shape[0])
                cols = w.shape[1] if base == 'to_feat' else pad64(w.shape[1])
                wo, bo = np.zeros((rows, cols) + w.shape[2:], np.float32), np.zeros(rows, np.float32)
                wo[:w.shape[0], :w.shape[1]], bo[:b.shape[0]] = w, b
                w, b = wo, bo
            cache[base] = (w, b)
        w, b = cache[base]
        if not p:
            return w, b
        rows = slice(64 * int(p), 64 * int(p) + 64)
        return w[rows], b[rows]

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        EngineModule._ensure_engine(self)
        self.__dict__.pop('_relayout_cache', None)
        sd = self.state_dict()
        f32 = lambda key: np.ascontiguousarray(sd[key].detach().float().cpu().numpy())
        for b in range(self.n_blocks):
            k = f'feats.{b}.'
            taps = np.ascontiguousarray(np.concatenate([f32(k + f'safm.mfr.{i}.weight').reshape(-1, 9) for i in range(4)]))
            bias = np.ascontiguousarray(np.concatenate([f32(k + f'safm.mfr.{i}.bias') for i in range(4)]))
            L.check(L.lib.innfer_net_set_safm(self._handle, b, taps.ctypes.data, bias.ctypes.data))
            for j, n in enumerate(('norm1', 'norm2')):
                g, be = f32(k + n + '.weight'), f32(k + n + '.bias')
                L.check(L.lib.innfer_net_set_layer_norm(self._handle, 2 * b + j, g.ctypes.data, be.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'SAFMN is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    @staticmethod
    def _check_size(H, W):
        if H < 8 or W < 8:
            raise NotImplementedError(f'SAFMN pools its features down to (H >> 3) x (W >> 3): both sides must be at least 8 pixels, got {H} x {W}')
