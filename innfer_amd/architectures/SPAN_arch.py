"""SPAN shell (Swift Parameter-free Attention Network, the NTIRE 2024 efficient-SR winner: most of the community's "fast" 2x / 4x models).  The reference has
no such architecture; constructor surface and state-dict keys are the published ones, the graph is built inside libinnfer_amd.so (csrc/net.hip, kind 3).

Conv3XC(ci, co, gain=2) holds (all with bias)

    sk = Conv2d(ci, co, 1); conv.0 = Conv2d(ci, ci gain, 1); conv.1 = Conv2d(ci gain, co gain, 3, padding=0); conv.2 = Conv2d(co gain, co, 1);
    eval_conv = Conv2d(ci, co, 3, padding=1)

and in eval mode is ONE 3x3 zero-pad-1 conv whose weights are recomputed from sk and conv.* in every forward (the stored eval_conv.* is overwritten there, it is
not the source of truth):

    W[o,i,y,x] = sum_{m,j} conv.2.w[o,m] conv.1.w[m,j,y,x] conv.0.w[j,i];   W[o,i,1,1] += sk.w[o,i]
    b[o]       = sum_m conv.2.w[o,m] (sum_{j,y,x} conv.1.w[m,j,y,x] conv.0.b[j] + conv.1.b[m]) + conv.2.b[o] + sk.b[o]

(equal to the training branch conv(F.pad(x, 1)) + sk(x) on the border too: the padded ring carries conv.0.b).

    SPAB(c): c1_r, c2_r, c3_r = Conv3XC(c, c)
        out1 = c1_r(x); out2 = c2_r(SiLU(out1)); out3 = c3_r(SiLU(out2)); out = (out3 + x) * (sigmoid(out3) - 0.5); returns (out, out1, gate)   # out1 PRE-activation

    SPAN: conv_1 = Conv3XC(in, f); block_1 .. block_6 = SPAB(f); conv_2 = Conv3XC(f, f); conv_cat = Conv2d(4 f, f, 1);
          upsampler.0 = Conv2d(f, out upscale^2, 3, 1, 1), PixelShuffle(upscale)
        x  = (x - mean) * img_range            # only when norm; per channel; the mean is NOT added back at the end (the published quirk)
        f0 = conv_1(x); b1 = block_1(f0)[0] .. b5 = block_5(b4)[0]; b6, b5_2, _ = block_6(b5)
        out = PixelShuffle(upscale)(upsampler.0(conv_cat(cat[f0, conv_2(b6), b1, b5_2])))

norm=False (the community training framework's variant) registers the one-element buffer `no_norm` its checkpoints carry; deploy=True registers only the
eval_conv.* keys and uses them as given.  The collapse runs on the host in float64 at upload and is rounded to fp32."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import span_convs, span_shapes


def collapse_conv3xc(sd, p):
    """(weight [co, ci, 3, 3], bias [co]) float32 of the one conv Conv3XC `p` is in eval mode, from sk and conv.* in float64 (the two formulas of the module docstring)."""
    g = lambda k: sd[f'{p}.{k}'].detach().double().cpu().numpy()
    w0, b0, w1, b1, w2, b2 = g('conv.0.weight')[:, :, 0, 0], g('conv.0.bias'), g('conv.1.weight'), g('conv.1.bias'), g('conv.2.weight')[:, :, 0, 0], g('conv.2.bias')
    w = np.einsum('om,mjyx,ji->oiyx', w2, w1, w0)
    w[:, :, 1, 1] += g('sk.weight')[:, :, 0, 0]
    b = w2 @ (np.einsum('mjyx,j->m', w1, b0) + b1) + b2 + g('sk.bias')
    return w.astype(np.float32), b.astype(np.float32)


class SPAN(EngineModule):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, num_in_ch=3, num_out_ch=3, feature_channels=48, upscale=4, bias=True, norm=True, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040), deploy=False):
        unsupported = []
        if not isinstance(feature_channels, int) or not 1 <= feature_channels <= 64: unsupported.append(f'feature_channels={feature_channels} (1..64)')
        if num_in_ch != num_out_ch or not 1 <= num_in_ch <= 4: unsupported.append(f'num_in_ch={num_in_ch}, num_out_ch={num_out_ch} (equal, 1..4)')
        if upscale not in (1, 2, 3, 4): unsupported.append(f'upscale={upscale} (1..4)')
        if norm and num_in_ch != len(rgb_mean): unsupported.append(f'norm with num_in_ch={num_in_ch} (rgb_mean has {len(rgb_mean)} entries)')
        if not bias: unsupported.append('bias=False')
        if unsupported:
            raise NotImplementedError('SPAN option(s) not built on the HIP path: ' + ', '.join(unsupported))
        shapes = span_shapes(num_in_ch, num_out_ch, feature_channels, upscale, norm, deploy)
        shapes.pop('no_norm', None)
        super().__init__(shapes)
        if not norm:
            self.register_buffer('no_norm', torch.zeros(1))
        self.in_nc, self.out_nc, self.nf, self.upscale = num_in_ch, num_out_ch, feature_channels, upscale
        self.norm, self.img_range, self.rgb_mean, self.deploy = bool(norm), float(img_range), tuple(float(m) for m in rgb_mean), bool(deploy)
        self.engine_nf = 32 if feature_channels <= 32 else 64          # the engine's feature width: fewer features are zero-padded on upload (exact: SiLU(0) = 0, gate(0, 0) = 0)
        self._units = set(span_convs())

    def _create_handle(self):
        h = C.c_void_p()
        mean = np.zeros(4, np.float32)
        if self.norm:
            mean[:self.in_nc] = self.rgb_mean
        L.check(L.lib.innfer_span_create(C.byref(h), self.in_nc, self.out_nc, self.engine_nf, self.upscale, int(self.norm), self.img_range, mean.ctypes.data))
        return h

    def _conv_tensors(self, k, sd):
        """The engine's conv `k`: the collapsed Conv3XC (or its eval_conv as given, `deploy`), conv_cat with its four f-wide input ranges spread to the engine's four
        nf-wide ones, upsampler.0 -- features zero-padded to the engine's width."""
        nf, f = self.engine_nf, self.nf
        if k in self._units:
            w, b = super()._conv_tensors(k + '.eval_conv', sd) if self.deploy else collapse_conv3xc(sd, k)
        else:
            w, b = super()._conv_tensors(k, sd)
        if f == nf:
            return w, b
        if k == 'conv_cat':
            wp = np.zeros((nf, 4 * nf, 1, 1), np.float32)
            for r in range(4):
                wp[:f, r * nf:r * nf + f] = w[:, r * f:(r + 1) * f]
        else:
            K = w.shape[0] if k == 'upsampler.0' else nf
            Cin = w.shape[1] if k == 'conv_1' else nf
            wp = np.zeros((K, Cin, 3, 3), np.float32)
            wp[:w.shape[0], :w.shape[1]] = w
        bp = np.zeros(wp.shape[0], np.float32)
        bp[:b.shape[0]] = b
        return wp, bp

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'SPAN is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    def forward(self, x, outm=None, out=None):
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            raise self._fp16_only('a float32 input was given')
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'SPAN has no outm ({outm!r})')
        return super().forward(x, None, out)

    def forward_u8(self, img, normalize=False, fp16=True, out=None):
        if not fp16:
            raise self._fp16_only('forward_u8(fp16=False) was asked for')
        return super().forward_u8(img, normalize, True, out)

    def tile_batch_bytes(self, b, ps, dtype=torch.float16, device=None):
        if dtype == torch.float32:
            raise self._fp16_only('float32 tiles were asked for')
        return super().tile_batch_bytes(b, ps, dtype, device)
