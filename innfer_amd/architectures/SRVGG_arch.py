"""BasicSR's SRVGGNetCompact shell (realesr-animevideov3, realesr-general-x4v3 and the community "compact" / "ultracompact" checkpoints).  The reference
has no such architecture; constructor surface and state-dict keys are BasicSR's, the graph is built inside libinnfer_amd.so (csrc/net.hip, kind 2):

    body.0 = Conv2d(num_in_ch, num_feat, 3, 1, 1), body.1 its activation; body.2i / body.2i+1 the num_conv convs num_feat -> num_feat and theirs;
    body.<2 num_conv + 2> = Conv2d(num_feat, num_out_ch * upscale^2, 3, 1, 1);   out = PixelShuffle(upscale)(body(x)) + nearest_upsample(x, upscale)

The activation (PReLU(num_feat) / ReLU / LeakyReLU(0.1)) is one code path of the engine: per-channel slopes in the conv's epilogue."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import compact_shapes

_ACTS = ('prelu', 'relu', 'leakyrelu')


class SRVGGNetCompact(EngineModule):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type='prelu'):
        unsupported = []
        if act_type not in _ACTS: unsupported.append(f'act_type={act_type}')
        if not isinstance(num_feat, int) or not 1 <= num_feat <= 64: unsupported.append(f'num_feat={num_feat} (1..64)')
        if num_in_ch != num_out_ch or not 1 <= num_in_ch <= 4: unsupported.append(f'num_in_ch={num_in_ch}, num_out_ch={num_out_ch} (equal, 1..4)')
        if not isinstance(num_conv, int) or num_conv < 0: unsupported.append(f'num_conv={num_conv}')
        if upscale not in (1, 2, 3, 4): unsupported.append(f'upscale={upscale} (1..4)')
        if unsupported:
            raise NotImplementedError('SRVGGNetCompact option(s) not built on the HIP path: ' + ', '.join(unsupported))
        super().__init__(compact_shapes(num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type))
        self.in_nc, self.out_nc, self.nf, self.num_conv, self.upscale, self.act_type = num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type
        self.engine_nf = 32 if num_feat <= 32 else 64          # the engine's feature width: fewer features are zero-padded on upload (exact)
        self._last = f'body.{2 * num_conv + 2}'

    def _create_handle(self):
        h = C.c_void_p()
        L.check(L.lib.innfer_compact_create(C.byref(h), self.in_nc, self.out_nc, self.engine_nf, self.num_conv, self.upscale))
        return h

    def _conv_tensors(self, k, sd):
        """Weights and bias zero-padded to the engine's feature width: a padded feature is conv(0 weights) + 0 bias -> 0, slope 0, and meets zero weights downstream."""
        w, b = super()._conv_tensors(k, sd)
        nf, f = self.engine_nf, self.nf
        if f == nf:
            return w, b
        K = w.shape[0] if k == self._last else nf
        Cin = w.shape[1] if k == 'body.0' else nf
        wp = np.zeros((K, Cin, 3, 3), np.float32)
        wp[:w.shape[0], :w.shape[1]] = w
        bp = np.zeros(K, np.float32)
        if b is not None:
            bp[:b.shape[0]] = b
        return wp, bp

    def _slopes(self, k, sd):
        """The engine_nf slopes of the activation behind conv `k`: y = x if x >= 0 else slope[c] * x."""
        s = np.zeros(self.engine_nf, np.float32)
        if self.act_type == 'prelu':
            a = sd[f'body.{int(k.split(".")[1]) + 1}.weight'].detach().float().cpu().numpy()
            s[:a.shape[0]] = a
        elif self.act_type == 'leakyrelu':
            s[:self.nf] = 0.1
        return s

    def _ensure_engine(self):
        ver = self._weights_version()
        if self._handle is not None and ver == self._uploaded_version:
            return
        super()._ensure_engine()
        sd = self.state_dict()
        key = C.create_string_buffer(128)
        K, Cc = C.c_int(), C.c_int()
        for i in range(L.lib.innfer_net_num_convs(self._handle)):
            L.check(L.lib.innfer_net_conv_info(self._handle, i, key, 128, C.byref(K), C.byref(Cc)))
            k = key.value.decode()
            if k != self._last:
                s = self._slopes(k, sd)
                L.check(L.lib.innfer_net_set_conv_slope(self._handle, i, s.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'SRVGGNetCompact is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    def forward(self, x, outm=None, out=None):
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            raise self._fp16_only('a float32 input was given')
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'SRVGGNetCompact has no outm ({outm!r})')
        return super().forward(x, None, out)

    def forward_u8(self, img, normalize=False, fp16=True, out=None):
        if not fp16:
            raise self._fp16_only('forward_u8(fp16=False) was asked for')
        return super().forward_u8(img, normalize, True, out)

    def tile_batch_bytes(self, b, ps, dtype=torch.float16, device=None):
        if dtype == torch.float32:
            raise self._fp16_only('float32 tiles were asked for')
        return super().tile_batch_bytes(b, ps, dtype, device)
