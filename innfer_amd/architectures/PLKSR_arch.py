"""RealPLKSR shell (partial large-kernel convolution network for super-resolution, the "Real" variant with GroupNorm: a family of the community's 2x / 4x models).
The reference has no such architecture; constructor surface and state-dict keys are the published ones, the graph is built inside libinnfer_amd.so (csrc/net.hip,
kind 4; csrc/plk_conv.hip, csrc/group_norm.hip).

    DCCM(dim):       Sequential(Conv2d(dim, 2 dim, 3, 1, 1), Mish(), Conv2d(2 dim, dim, 3, 1, 1))
    PLKConv2d(p, k): conv = Conv2d(p, p, k, 1, k // 2);  forward: x[:, :p] = conv(x[:, :p])  (the other channels pass through)
    EA(dim):         f = Sequential(Conv2d(dim, dim, 3, 1, 1), Sigmoid());  forward: x * f(x)
    PLKBlock:        channel_mixer = DCCM(dim); lk = PLKConv2d(int(dim * split_ratio), k); attn = EA(dim) or Identity (use_ea False);
                     refine = Conv2d(dim, dim, 1); norm = GroupNorm(norm_groups, dim)       (eps 1e-5, biased variance, per sample over (dim / groups) x H x W)
                     forward: norm(refine(attn(lk(channel_mixer(x))))) + x
    RealPLKSR(in_ch 3, out_ch 3, dim 64, n_blocks 28, upscaling_factor 4, kernel_size 17, split_ratio 0.25, use_ea True, norm_groups 4):
                     feats = Sequential(Conv2d(in_ch, dim, 3, 1, 1), n_blocks x PLKBlock, Dropout2d (no parameters), Conv2d(dim, out_ch s^2, 3, 1, 1))
                     forward: PixelShuffle(s)(feats(x) + repeat_interleave(x, s^2, dim=1))
    Mish(f) = f * tanh(softplus(f)) = f * (n^2 + 2 n) / (n^2 + 2 n + 2),  n = exp(f)

The "S" variant is n_blocks 12, kernel_size 13, use_ea False.  norm_groups is a constructor argument: it leaves no trace in the keys.

GroupNorm's statistics are those of whatever tensor the network is given, per sample: a tiling front end (the 200-px chop of Model.run, `-tile N`) normalises every tile
by its own statistics, as every tiling front end does with this family; `-tile 0` or large tiles are the faithful setting."""
import ctypes as C

import numpy as np
import torch

from .. import lib as L
from .engine_module import EngineModule
from .keys import realplksr_shapes


class RealPLKSR(EngineModule):
    _has_fp32 = False        # the fp16 engine only: a float32 tensor / -no_fp16 is refused, never served with fp16 accuracy

    def __init__(self, in_ch=3, out_ch=3, dim=64, n_blocks=28, upscaling_factor=4, kernel_size=17, split_ratio=0.25, use_ea=True, norm_groups=4, dysample=False, **unused):
        unsupported = []
        p = int(dim * split_ratio) if isinstance(dim, int) else -1
        if dim != 64: unsupported.append(f'dim={dim} (64)')
        if p != 16: unsupported.append(f'split_ratio={split_ratio} (int(dim * split_ratio) = {p}; built: 16 channels under the large kernel)')
        if not isinstance(kernel_size, int) or kernel_size % 2 == 0 or not 3 <= kernel_size <= 17: unsupported.append(f'kernel_size={kernel_size} (odd, 3..17)')
        if out_ch != in_ch or not 1 <= in_ch <= 4: unsupported.append(f'in_ch={in_ch}, out_ch={out_ch} (equal, 1..4)')
        if upscaling_factor not in (1, 2, 3, 4): unsupported.append(f'upscaling_factor={upscaling_factor} (1..4)')
        if not isinstance(n_blocks, int) or n_blocks < 1: unsupported.append(f'n_blocks={n_blocks}')
        if norm_groups not in (1, 2, 4, 8): unsupported.append(f'norm_groups={norm_groups} (1, 2, 4, 8)')
        if dysample: unsupported.append('dysample=True')
        if unsupported:
            raise NotImplementedError('RealPLKSR option(s) not built on the HIP path: ' + ', '.join(unsupported))
        super().__init__(realplksr_shapes(in_ch, out_ch, dim, n_blocks, upscaling_factor, kernel_size, split_ratio, use_ea))
        self.in_nc, self.out_nc, self.nf, self.n_blocks, self.upscale = in_ch, out_ch, dim, n_blocks, upscaling_factor
        self.kernel_size, self.use_ea, self.norm_groups = kernel_size, bool(use_ea), norm_groups

    def _create_handle(self):
        h = C.c_void_p()
        L.check(L.lib.innfer_plksr_create(C.byref(h), self.in_nc, self.out_nc, self.nf, self.n_blocks, self.upscale, self.kernel_size, int(self.use_ea), self.norm_groups))
        return h

    def _conv_tensors(self, k, sd):
        """The engine runs channel_mixer.0 (dim -> 2 dim) as two 64-output launches: its keys `.0a` / `.0b` are output channels 0 .. 63 / 64 .. 127 of that conv."""
        if k.endswith('.channel_mixer.0a') or k.endswith('.channel_mixer.0b'):
            w, b = super()._conv_tensors(k[:-1], sd)
            h = slice(0, self.nf) if k.endswith('a') else slice(self.nf, 2 * self.nf)
            return w[h], (None if b is None else b[h])
        return super()._conv_tensors(k, sd)

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
            if k.endswith('.refine'):
                blk = k[:-len('.refine')]
                g = np.ascontiguousarray(sd[blk + '.norm.weight'].detach().float().cpu().numpy())
                b = np.ascontiguousarray(sd[blk + '.norm.bias'].detach().float().cpu().numpy())
                L.check(L.lib.innfer_net_set_group_norm(self._handle, i, g.ctypes.data, b.ctypes.data))

    @staticmethod
    def _fp16_only(what):
        return NotImplementedError(f'RealPLKSR is built for the fp16 mode only: {what} (no fp32-accurate engine; pass a float16 tensor / drop -no_fp16)')

    def forward(self, x, outm=None, out=None):
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            raise self._fp16_only('a float32 input was given')
        if outm is not None and outm in self._OUTM:
            raise NotImplementedError(f'RealPLKSR has no outm ({outm!r})')
        return super().forward(x, None, out)

    def forward_u8(self, img, normalize=False, fp16=True, out=None):
        if not fp16:
            raise self._fp16_only('forward_u8(fp16=False) was asked for')
        return super().forward_u8(img, normalize, True, out)

    def tile_batch_bytes(self, b, ps, dtype=torch.float16, device=None):
        if dtype == torch.float32:
            raise self._fp16_only('float32 tiles were asked for')
        return super().tile_batch_bytes(b, ps, dtype, device)
