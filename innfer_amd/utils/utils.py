"""Mirror of the hot-path functions of the reference's utils/utils.py, backed by
HIP kernels (csrc/tiles.hip) through the C ABI:

    extract_patches_2d / recompose_tensor   utils/utils.py:318-369 / 372-445
    np2tensor / tensor2np                   utils/utils.py:164-194 / 197-248
    mod2normal / swa2normal                 utils/utils.py:666-698 / 701-720 (host, key renaming)

Same names, argument meaning and error behaviour.  Tensors must live on the
GPU; there is no CPU fallback.
"""
import functools
import os
import os.path as osp

import numpy as np
import torch

from .. import lib as L
from .defaults import SEAMLESS_PAD

try:                                    # the reference reads / writes through OpenCV (utils.py:3-4,68-95); PIL is the stand-in where it is absent
    import cv2
    cv2_available = True
except ImportError:
    cv2_available = False

IMG_EXTENSIONS = ['.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.webp', 'tga', '.tif', '.tiff', '.dng']       # utils.py:18-19 (sic: 'tga')
MODEL_EXTENSIONS = ['.pth', '.pt']                                                                       # utils.py:16

# what an integer image is divided by (utils.py:22-33; the image reader returns uint8 or uint16)
MAX_VALUES_BY_DTYPE = {np.dtype("uint8"): 255, np.dtype("uint16"): 65535}


def _dt(t):
    if t.dtype == torch.float16:
        return L.F16
    if t.dtype == torch.float32:
        return L.F32
    raise TypeError(f'unsupported dtype {t.dtype}')


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: tensor must be on the GPU (innfer_amd has no CPU path)')


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _on(t):
    """The library launches on the process's current HIP device: make it the tensor's for the call."""
    return torch.cuda.device(t.device)


def extract_patches_2d(img, patch_shape, step=None, batch_first=False, tile_range=None):
    """[1,C,H,W] -> [n,1,C,ph,pw] ([1,n,C,ph,pw] when batch_first): sliding tiles
    with stride int(patch*step) plus a ragged last row/column (utils.py:318-369).
    tile_range=(begin,count) extracts a contiguous sub-range (multi-GPU sharding)."""
    if step is None:
        step = [1.0, 1.0]
    _need_cuda(img, 'extract_patches_2d')
    B, C, H, W = img.shape
    ph, pw = patch_shape
    if B != 1:
        raise NotImplementedError('extract_patches_2d: batch > 1 (run.py only ever passes batch 1)')
    if ph != pw or step[0] != step[1] or not isinstance(step[0], float):
        raise NotImplementedError('extract_patches_2d: square patches with one fractional step only (chop_forward usage)')
    if H < ph or W < pw:
        # the reference's pad branch dereferences an undefined name `nn` (utils.py:341,346)
        raise NameError("name 'nn' is not defined")
    ps, ys, xs = L.chop_plan(H, W, ph, step[0])
    n = len(ys) * len(xs)
    begin, count = tile_range if tile_range is not None else (0, n)
    img = img.contiguous()
    tiles = torch.empty((count, C, ps, ps), dtype=img.dtype, device=img.device)
    with _on(img):
        L.check(L.lib.innfer_extract_tiles(img.data_ptr(), _dt(img), C, H, W, ph, step[0], begin, count,
                                       tiles.data_ptr(), _stream(img)))
    out = tiles.unsqueeze(1)                       # [n, B=1, C, ph, pw]
    return out.permute(1, 0, 2, 3, 4) if batch_first else out


def recompose_tensor(patches, height, width, step=None, scale=1, out_dtype=None):
    """Weighted overlap blend of [n,C,P,P] tiles into [n/(nh*nw),C,scale*H,scale*W]
    (utils.py:372-445).  fp32 accumulation in the reference's tile order."""
    if step is None:
        step = [1.0, 1.0]
    assert isinstance(step, float) and step >= 0.5 and step <= 1.0
    _need_cuda(patches, 'recompose_tensor')
    patches = patches.contiguous()
    n, C, P, P2 = patches.shape
    assert P == P2
    FH, FW = scale * height, scale * width
    eff = int(P * step)
    nh = 1 + (max(FH, P) - P) // eff + (1 if (max(FH, P) - P) % eff else 0)
    nw = 1 + (max(FW, P) - P) // eff + (1 if (max(FW, P) - P) % eff else 0)
    nb = n // (nh * nw)
    dtype = out_dtype or patches.dtype
    out = torch.empty((nb, C, FH, FW), dtype=dtype, device=patches.device)
    odt = L.F16 if dtype == torch.float16 else L.F32
    with _on(patches):
        L.check(L.lib.innfer_recompose(patches.data_ptr(), _dt(patches), n, C, P, height, width, float(step), scale,
                                       out.data_ptr(), odt, _stream(patches)))
    return out


def np2tensor(img, bgr2rgb=True, data_range=1., normalize=False, change_range=True, add_batch=True,
              device='cuda', dtype=torch.float32):
    """uint8 / uint16 HWC BGR(A) image -> [1,C,H,W] RGB(A) float tensor ON THE GPU
    (utils.py:164-194): the integer image crosses PCIe (4x / 2x fewer bytes than fp32) and
    /maxval (MAX_VALUES_BY_DTYPE, utils.py:22-33), HWC->CHW, channel flip and optional [-1,1] norm run in one HIP kernel.
    bgr2rgb / change_range / add_batch as in the reference (`data_range` is unused there too)."""
    if not isinstance(img, np.ndarray):
        raise TypeError("Got unexpected object type, expected np.ndarray")
    if img.dtype not in (np.uint8, np.uint16) or img.ndim != 3:
        raise NotImplementedError('np2tensor: uint8 / uint16 HWC images are built (the reader, utils.py:36-133, produces nothing else)')
    H, W, Cc = img.shape
    bits = 8 if img.dtype == np.uint8 else 16
    maxval = float(MAX_VALUES_BY_DTYPE[img.dtype]) if change_range else 1.0
    host = np.ascontiguousarray(img)
    if bits == 16:                                   # torch has no uint16 arithmetic; the bytes are what crosses PCIe
        host = host.view(np.int16)
    d_img = torch.from_numpy(host).to(device)
    out = torch.empty((1, Cc, H, W), dtype=dtype, device=d_img.device)
    with _on(out):
        L.check(L.lib.innfer_inthwc_to_nchw(d_img.data_ptr(), bits, H, W, Cc, int(bool(bgr2rgb)), int(bool(normalize)), maxval,
                                            out.data_ptr(), _dt(out), _stream(out)))
    return out if add_batch else out.squeeze(0)


def tensor2np(img, rgb2bgr=True, remove_batch=True, data_range=255, denormalize=False,
              change_range=True, imtype=np.uint8):
    """[1,C,H,W] / [C,H,W] / [H,W] RGB float GPU tensor -> HWC BGR uint8 (or uint16) numpy (utils.py:197-248);
    clip * data_range and round-half-to-even on the GPU, one integer D2H copy.  (data_range, imtype) = (255, np.uint8) or
    (65535, np.uint16); rgb2bgr as in the reference (3- and 4-channel images only)."""
    if not isinstance(img, torch.Tensor):
        raise TypeError("Got unexpected object type, expected torch.Tensor")
    n_dim = img.dim()
    if n_dim not in (2, 3, 4):
        raise TypeError(f'Only support 4D, 3D and 2D tensor. But received with dimension: {n_dim:d}')
    if n_dim == 4 and (img.shape[0] != 1 or not remove_batch):
        raise NotImplementedError('tensor2np: a 4D tensor must be one image with remove_batch=True (the reference transposes a kept batch axis into the image)')
    if not change_range or (data_range, np.dtype(imtype)) not in ((255, np.dtype(np.uint8)), (65535, np.dtype(np.uint16))):
        raise NotImplementedError('tensor2np: built for (data_range, imtype) = (255, uint8) and (65535, uint16) with change_range=True')
    _need_cuda(img, 'tensor2np')
    img = img.contiguous()
    Cc, (H, W) = (1 if n_dim == 2 else img.shape[-3]), img.shape[-2:]
    bits = 8 if np.dtype(imtype) == np.dtype(np.uint8) else 16
    out = torch.empty((H, W, Cc), dtype=torch.uint8 if bits == 8 else torch.int16, device=img.device)
    with _on(img):
        L.check(L.lib.innfer_nchw_to_inthwc(img.data_ptr(), _dt(img), H, W, Cc, int(bool(rgb2bgr) and n_dim != 2), int(bool(denormalize)), bits,
                                            out.data_ptr(), _stream(img)))
    arr = out.cpu().numpy()
    if bits == 16:
        arr = arr.view(np.uint16)
    return arr[:, :, 0] if n_dim == 2 else arr


# ---------------------------------------------------------------- fit_channels: gray, gray + alpha and BGRA images through an RGB network
# The colour plane goes through the network as (g, g, g) or RGB, the alpha plane as (a, a, a); a gray or alpha result is mean3 of the network's
# three channels, ((y0 + y1) + y2) / 3 in fp32 rounded to the result dtype, quantised as tensor2np.  A constant alpha plane is not run: its value is
# copied.  Kernels: csrc/tiles.hip, csrc/tiles_u8.hip (include/innfer_amd.h, ABI 115).  The reference runs such images as they are and fails (utils.py:164-248).

def fit_channels_plan(shape, dtype, in_nc, out_nc):
    """How Model.run_u8(fit_channels=True) / `-fit_channels` run an image of `shape` (HWC or HW) with an in_nc -> out_nc network:
    1, 2 or 4 -- the image's channel count (2-D = 1): colour (+ alpha) through a 3 -> 3 network; 0 -- a 2-D image for an in_nc == 1 network,
    run as H x W x 1; None -- the image does not qualify and goes the way it goes without the switch (an image that already has in_nc channels,
    a network that is not 3 -> 3, any other channel count)."""
    nd = len(shape)
    if nd == 2 and in_nc == 1:
        plan = 0
    elif in_nc == 3 and out_nc == 3 and (nd == 2 or (nd == 3 and shape[2] in (1, 2, 4))):
        plan = 1 if nd == 2 else int(shape[2])
    else:
        return None
    if np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise NotImplementedError(f'fit_channels: uint8 / uint16 images are built, got {np.dtype(dtype)}')
    return plan


def fit_channels_out_shape(shape, scale):
    """Shape of the image fit_channels returns for an input of `shape` (HW or HWC) and a network of `scale`: the input's layout at scale x the size."""
    return (shape[0] * scale, shape[1] * scale) + tuple(shape[2:])


def _bits(t):
    return 8 if t.dtype == torch.uint8 else 16


def alpha_constant(d_img, C):
    """The value of the alpha plane (the last channel) of the [H, W, C] uint8 / int16-viewed uint16 GPU image when it is one value everywhere,
    else None: min and max on the GPU, one 8-byte readback."""
    H, W = d_img.shape[:2]
    mm = torch.empty(2, dtype=torch.int32, device=d_img.device)
    with _on(d_img):
        L.check(L.lib.innfer_channel_minmax(d_img.data_ptr(), _bits(d_img), H, W, C, C - 1, mm.data_ptr(), _stream(d_img)))
    lo, hi = mm.tolist()
    return lo if lo == hi else None


def fit_split(d_img, normalize=False, dtype=torch.float32):
    """np2tensor of the two planes of an [H, W] / [H, W, C] (C 1, 2, 4) uint8 / int16-viewed uint16 GPU image:
    (colour [1, 3, H, W], alpha [1, 3, H, W] or None, alpha_const or None).  alpha is None when the image has no alpha plane or a constant one."""
    x = d_img.contiguous()
    H, W = x.shape[:2]
    C = x.shape[2] if x.dim() == 3 else 1
    const = alpha_constant(x, C) if C in (2, 4) else None
    colour = torch.empty((1, 3, H, W), dtype=dtype, device=x.device)
    alpha = torch.empty_like(colour) if C in (2, 4) and const is None else None
    maxval = 255.0 if _bits(x) == 8 else 65535.0
    with _on(x):
        L.check(L.lib.innfer_inthwc_to_nchw_fit(x.data_ptr(), _bits(x), H, W, C, int(bool(normalize)), maxval, colour.data_ptr(),
                                                alpha.data_ptr() if alpha is not None else None, _dt(colour), _stream(x)))
    return colour, alpha, const


def fit_merge(colour, alpha, alpha_const, C, denormalize=False, bits=8, out=None):
    """tensor2np of the two results into the image's layout, on the GPU: colour / alpha [1, 3, H', W'] results of one dtype (alpha None when
    alpha_const holds the constant alpha, or C == 1) -> [H', W', C] uint8 (bits 8) or int16-viewed uint16 (bits 16) tensor (`out` if given)."""
    colour = colour.contiguous()
    if colour.dim() != 4 or colour.shape[:2] != (1, 3):
        raise ValueError(f'fit_merge: expected a [1, 3, H, W] result, got {tuple(colour.shape)}')
    if alpha is not None:
        alpha = alpha.contiguous()
        if alpha.shape != colour.shape or alpha.dtype != colour.dtype:
            raise ValueError('fit_merge: the alpha result must match the colour result in shape and dtype')
    H, W = colour.shape[2:]
    if out is None:
        out = torch.empty((H, W, C), dtype=torch.uint8 if bits == 8 else torch.int16, device=colour.device)
    with _on(colour):
        L.check(L.lib.innfer_nchw_to_inthwc_fit(colour.data_ptr(), alpha.data_ptr() if alpha is not None else None, _dt(colour), H, W, C,
                                                int(bool(denormalize)), bits, -1 if alpha_const is None else int(alpha_const), out.data_ptr(), _stream(colour)))
    return out


def fit_channels_forward(fn, img, normalize=False, device='cuda', dtype=torch.float32):
    """The tensor path of fit_channels (model chains, the guided filter, uint16 images): img, an HW / HWC (C 1, 2, 4) uint8 or uint16 numpy image,
    -> the same layout and dtype at the network's scale.  fn maps a [1, 3, H, W] tensor of `dtype` to the network's [1, 3, H', W'] result; it runs on
    the colour plane and, as its own call, on a non-constant alpha plane."""
    if not isinstance(img, np.ndarray) or img.ndim not in (2, 3):
        raise TypeError('fit_channels_forward: expected an HW / HWC numpy image')
    if fit_channels_plan(img.shape, img.dtype, 3, 3) is None:
        raise ValueError(f'fit_channels_forward: a {img.shape[2]}-channel image has no fit_channels layout (1, 2 or 4 channels)')
    host = np.ascontiguousarray(img)
    bits = 8 if host.dtype == np.uint8 else 16
    d_img = torch.from_numpy(host if bits == 8 else host.view(np.int16)).to(device)
    C = img.shape[2] if img.ndim == 3 else 1
    colour, alpha, const = fit_split(d_img, normalize=normalize, dtype=dtype)
    y = fn(colour)
    ya = fn(alpha) if alpha is not None else None
    arr = fit_merge(y, ya, const, C, denormalize=normalize, bits=bits).cpu().numpy()
    if bits == 16:
        arr = arr.view(np.uint16)
    return arr[:, :, 0] if img.ndim == 2 else arr


# ---------------------------------------------------------------- seamless modes: tileable textures without a seam at the border
# The image is run as if it had been padded by SEAMLESS_PAD pixels with its own continuation ('tile', 'mirror', 'replicate') or with transparent black
# ('alpha_pad') and the padding cut off the result.  Kernels: csrc/tiles_u8.hip (include/innfer_amd.h, ABI 117).  Not in the reference.
SEAMLESS_MODES = tuple(L.BORDER_MODES)
_NP_PAD_MODE = {'tile': 'wrap', 'mirror': 'reflect', 'replicate': 'edge', 'alpha_pad': 'constant'}


def seamless_mode(mode, H=None, W=None):
    """The INNFER_BORDER_* code of a seamless mode name; ValueError for an unknown name and for 'mirror' on an image with a side of one pixel."""
    if mode not in L.BORDER_MODES:
        raise ValueError(f"seamless: mode must be one of {', '.join(SEAMLESS_MODES)}, got {mode!r}")
    if mode == 'mirror' and H is not None and (H < 2 or W < 2):
        raise ValueError(f"seamless: 'mirror' needs at least 2 rows and 2 columns, the image is {H}x{W}")
    return L.BORDER_MODES[mode]


def seamless_pad_np(img, mode, pad=SEAMLESS_PAD):
    """The contract of the seamless modes in numpy: the HW / HWC image padded by `pad` pixels on every side of its two image axes, all channels alike --
    np.pad modes 'wrap' (tile), 'reflect' (mirror), 'edge' (replicate), zeros (alpha_pad)."""
    seamless_mode(mode, img.shape[0], img.shape[1])
    width = ((pad, pad), (pad, pad)) + ((0, 0),) * (img.ndim - 2)
    return np.pad(img, width, mode=_NP_PAD_MODE[mode])


def seamless_pad(img, mode, pad=SEAMLESS_PAD):
    """seamless_pad_np on the GPU (innfer_pad_inthwc): img is an HW / HWC uint8 or uint16 numpy image (a numpy image comes back) or a uint8 / int16-viewed
    uint16 GPU tensor (a GPU tensor comes back)."""
    host = isinstance(img, np.ndarray)
    if img.ndim not in (2, 3):
        raise TypeError('seamless_pad: expected an HW / HWC image')
    H, W = img.shape[:2]
    code = seamless_mode(mode, H, W)
    if host:
        if img.dtype not in (np.uint8, np.uint16):
            raise TypeError(f'seamless_pad: uint8 / uint16 images, got {img.dtype}')
        a = np.ascontiguousarray(img)
        d = torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()
    else:
        if img.dtype not in (torch.uint8, torch.int16):
            raise TypeError(f'seamless_pad: uint8 / int16-viewed uint16 tensors, got {img.dtype}')
        _need_cuda(img, 'seamless_pad')
        d = img.contiguous()
    Cc = d.shape[2] if d.dim() == 3 else 1
    out = torch.empty((H + 2 * pad, W + 2 * pad) + tuple(d.shape[2:]), dtype=d.dtype, device=d.device)
    with _on(d):
        L.check(L.lib.innfer_pad_inthwc(d.data_ptr(), _bits(d), H, W, Cc, pad, code, out.data_ptr(), _stream(d)))
    if not host:
        return out
    arr = out.cpu().numpy()
    return arr.view(np.uint16) if img.dtype == np.uint16 else arr


def seamless_crop(img_out, scale, pad=SEAMLESS_PAD):
    """The result of a padded image without its padding: scale * pad pixels off every side of an HW / HWC numpy image or GPU tensor (a contiguous copy)."""
    c = int(scale) * pad
    H, W = img_out.shape[:2]
    if H <= 2 * c or W <= 2 * c:
        raise ValueError(f'seamless_crop: nothing is left of {H}x{W} after {c} pixels off every side')
    r = img_out[c:H - c, c:W - c]
    return np.ascontiguousarray(r) if isinstance(img_out, np.ndarray) else r.contiguous()


# ---------------------------------------------------------------- self-ensemble (-tta): the eight dihedral orientations, averaged before quantisation
# t_k, k = 0 .. 7: transpose (H, W) if k & 4, then flip the columns if k & 1, then flip the rows if k & 2; t_k^-1 undoes the steps in reverse order.
# Kernels: csrc/tiles_tta.hip (include/innfer_amd.h, ABI 119); the tensor form is run.Model.forward_tta.  Not in the reference.

def _image_axes(img):
    """(row axis, column axis) of an HW / HWC numpy image or of a torch tensor, whose image axes are its last two (NCHW, CHW, HW)."""
    if isinstance(img, np.ndarray):
        if img.ndim not in (2, 3):
            raise TypeError('dihedral: expected an HW / HWC numpy image')
        return 0, 1
    if not isinstance(img, torch.Tensor) or img.dim() < 2:
        raise TypeError('dihedral: expected a numpy image or a tensor with at least two axes')
    return img.dim() - 2, img.dim() - 1


def _check_k(k):
    if not 0 <= int(k) <= 7:
        raise ValueError(f'dihedral: orientation k must be 0 .. 7, got {k}')
    return int(k)


def dihedral(img, k):
    """t_k of an HW / HWC numpy image or of a tensor (its last two axes): a contiguous copy."""
    k = _check_k(k)
    r, c = _image_axes(img)
    host = isinstance(img, np.ndarray)
    if k & 4:
        img = np.swapaxes(img, r, c) if host else img.transpose(r, c)
    if k & 1:
        img = np.flip(img, c) if host else img.flip(c)
    if k & 2:
        img = np.flip(img, r) if host else img.flip(r)
    return np.ascontiguousarray(img) if host else img.contiguous()


def dihedral_inv(img, k):
    """t_k^-1: dihedral_inv(dihedral(a, k), k) == a."""
    k = _check_k(k)
    r, c = _image_axes(img)
    host = isinstance(img, np.ndarray)
    if k & 2:
        img = np.flip(img, r) if host else img.flip(r)
    if k & 1:
        img = np.flip(img, c) if host else img.flip(c)
    if k & 4:
        img = np.swapaxes(img, r, c) if host else img.transpose(r, c)
    return np.ascontiguousarray(img) if host else img.contiguous()


def tta_np(fn, img):
    """The self-ensemble of a host function over a numpy image, the definition in numpy: the float32 sum of t_k^-1(fn(t_k(img))) in the order
    k = 0 .. 7, times 0.125, in fn's result dtype.  For tests on the CPU."""
    acc = None
    for k in range(8):
        y = dihedral_inv(np.asarray(fn(dihedral(img, k))), k)
        acc = y.astype(np.float32) if acc is None else acc + y.astype(np.float32)
    return (acc * np.float32(0.125)).astype(y.dtype)


# ---------------------------------------------------------------- resampling to any final size (-outscale)
# An antialiased separable resampler in the Pillow / ATen antialias=True convention (include/innfer_amd.h, ABI 118; csrc/resample.hip).  Channels are
# filtered independently: alpha is straight, NOT premultiplied, so colour under a transparent pixel does bleed into its neighbours' colour.  Not in the reference.
RESAMPLE_FILTERS = tuple(L.RESAMPLE_FILTERS)


def resample_size(h, w, scale):
    """The size of an h x w image at `scale`, by Real-ESRGAN's rule: max(1, int(h scale)) x max(1, int(w scale)).  ValueError unless 0 < scale < inf."""
    scale = float(scale)
    if not (scale > 0 and scale != float('inf')):
        raise ValueError(f'resample: the scale must be a positive finite number, got {scale!r}')
    return max(1, int(h * scale)), max(1, int(w * scale))


def _resample_axis0_np(x, plan, wrap):
    """One pass along axis 0 of the float32 array x: acc = acc + w * x per tap in ascending order, every operation rounded to float32."""
    start, count, weights = plan
    n = x.shape[0]
    acc = np.zeros((len(start),) + x.shape[1:], np.float32)
    tail = (1,) * (x.ndim - 1)
    for t in range(weights.shape[1]):                       # behind count[i] the weight is +0: acc + 0 * x == acc
        idx = start.astype(np.int64) + t
        idx = idx % n if wrap else np.clip(idx, 0, n - 1)
        acc = acc + weights[:, t].reshape((-1,) + tail) * x[idx]
    return acc


def resample_np(img, oh, ow, filter='lanczos', wrap=False):
    """The contract of the resampler in numpy: the HW / HWC uint8 or uint16 image at oh x ow, built from innfer_resample_plan's tables -- the
    horizontal pass, then the vertical one, float32 throughout, taps in ascending order, the code clamp(floor(acc + 0.5), 0, maxval)."""
    if not isinstance(img, np.ndarray) or img.ndim not in (2, 3) or img.dtype not in (np.uint8, np.uint16):
        raise TypeError('resample_np: expected an HW / HWC uint8 or uint16 numpy image')
    h, w = img.shape[:2]
    x = img.astype(np.float32)
    x = np.swapaxes(_resample_axis0_np(np.swapaxes(x, 0, 1), L.resample_plan(w, ow, filter, wrap), wrap), 0, 1)
    x = _resample_axis0_np(np.ascontiguousarray(x), L.resample_plan(h, oh, filter, wrap), wrap)
    maxval = 255 if img.dtype == np.uint8 else 65535
    return np.clip(np.floor(x + np.float32(0.5)), 0, maxval).astype(img.dtype)


@functools.lru_cache(maxsize=64)
def _resample_plan_dev(n_in, n_out, code, wrap, device):
    """The plan of one axis on `device`, uploaded once per (n_in, n_out, filter, wrap): (start, count, weights, T)."""
    start, count, weights = L.resample_plan(n_in, n_out, code, wrap)
    return tuple(torch.from_numpy(a).to(device) for a in (start, count, weights)) + (weights.shape[1],)


def resample(img, size=None, scale=None, filter='lanczos', wrap=False, out=None):
    """resample_np on the GPU (innfer_resample_inthwc): img is an HW / HWC (C 1 .. 4) uint8 or uint16 numpy image (a numpy image comes back) or a uint8 /
    int16-viewed uint16 GPU tensor (a GPU tensor comes back).  size = (oh, ow), or scale: resample_size.  wrap: taps wrap around, for tileable textures.
    A target equal to the source size returns img itself: no kernel runs.  out: a contiguous GPU tensor of the result's shape to write into."""
    host = isinstance(img, np.ndarray)
    if img.ndim not in (2, 3):
        raise TypeError('resample: expected an HW / HWC image')
    if (size is None) == (scale is None):
        raise ValueError('resample: give exactly one of size and scale')
    h, w = img.shape[:2]
    oh, ow = resample_size(h, w, scale) if size is None else (int(size[0]), int(size[1]))
    code = L.resample_filter(filter)
    if oh < 1 or ow < 1:
        raise ValueError(f'resample: bad size {oh}x{ow}')
    if (oh, ow) == (h, w) and out is None:
        return img
    if host:
        if img.dtype not in (np.uint8, np.uint16):
            raise TypeError(f'resample: uint8 / uint16 images, got {img.dtype}')
        a = np.ascontiguousarray(img)
        d = torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()
    else:
        if img.dtype not in (torch.uint8, torch.int16):
            raise TypeError(f'resample: uint8 / int16-viewed uint16 tensors, got {img.dtype}')
        _need_cuda(img, 'resample')
        d = img.contiguous()
    Cc = d.shape[2] if d.dim() == 3 else 1
    shape = (oh, ow) + tuple(d.shape[2:])
    if out is None:
        out = torch.empty(shape, dtype=d.dtype, device=d.device)
    elif tuple(out.shape) != shape or out.dtype != d.dtype or out.device != d.device or not out.is_contiguous():
        raise ValueError(f'resample: out must be a contiguous {d.dtype} tensor of shape {shape} on {d.device}')
    if (oh, ow) == (h, w):
        out.copy_(d)
        return out
    wrap = bool(wrap)
    hs, hc, hw, Th = _resample_plan_dev(w, ow, code, wrap, d.device)
    vs, vc, vw, Tv = _resample_plan_dev(h, oh, code, wrap, d.device)
    nbytes = L.lib.innfer_resample_workspace_bytes(h, w, Cc, oh, ow, Th, Tv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d.device) if nbytes else None
    with _on(d):
        L.check(L.lib.innfer_resample_inthwc(d.data_ptr(), _bits(d), h, w, Cc, out.data_ptr(), oh, ow, hs.data_ptr(), hc.data_ptr(), hw.data_ptr(), Th,
                                             vs.data_ptr(), vc.data_ptr(), vw.data_ptr(), Tv, int(wrap), ws.data_ptr() if nbytes else None, nbytes, _stream(d)))
    if not host:
        return out
    arr = out.cpu().numpy()
    return arr.view(np.uint16) if img.dtype == np.uint16 else arr


# ---------------------------------------------------------------- files (utils.py:36-133): the image loop's codec hand-off
def _suffixes(extensions):
    return tuple(extensions) if not isinstance(extensions, str) else (extensions,)


def is_ext_file(filename, extensions=IMG_EXTENSIONS):
    """True when the name ends in one of `extensions` (case-sensitive, as the reference's lists spell both cases: utils.py:36-37)."""
    return os.fspath(filename).endswith(_suffixes(extensions))


def scan_dir(path, extensions=IMG_EXTENSIONS):
    """Every file below `path` whose name ends in one of `extensions`, ordered by (directory, name) -- the order of the reference's sorted walk
    (utils.py:40-49), which is the order the image loop processes and numbers its outputs in."""
    if not osp.isdir(path):
        raise AssertionError(f'{path:s} is not a valid directory')
    suffixes = _suffixes(extensions)
    hits = [(folder, name) for folder, _, names in os.walk(path) for name in names if name.endswith(suffixes)]
    return [osp.join(folder, name) for folder, name in sorted(hits)]


def _non_empty_scan(path, extensions, what):
    found = scan_dir(path, extensions)
    if not found:
        raise AssertionError(f'{path:s} has no valid {what} file')
    return found


def get_models_paths(path):
    return _non_empty_scan(path, MODEL_EXTENSIONS, 'model')


def get_images_paths(path):
    return _non_empty_scan(path, IMG_EXTENSIONS, 'image')


def read_img(path=None):
    """cv2.imread(path, IMREAD_UNCHANGED) (utils.py:68-89): HWC BGR / BGRA (HW for gray), uint8 or uint16, None when the file cannot
    be decoded.  Without OpenCV the file is decoded by PIL and put into OpenCV's channel order."""
    if not path:
        raise AssertionError("Empty path provided.")
    if cv2_available:
        return cv2.imread(path, cv2.IMREAD_UNCHANGED)
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode in ('P', 'CMYK', 'YCbCr', '1'):
                im = im.convert('RGBA' if 'transparency' in im.info else 'RGB')
            elif im.mode == 'LA':
                im = im.convert('RGBA')
            a = np.asarray(im)
    except Exception:
        return None
    if a.dtype == np.int32:                  # PIL's 16-bit gray ('I') arrives as int32
        a = a.astype(np.uint16)
    if a.ndim == 3 and a.shape[2] == 3:
        a = a[:, :, ::-1]
    elif a.ndim == 3 and a.shape[2] == 4:
        a = a[:, :, [2, 1, 0, 3]]
    return np.ascontiguousarray(a)


def _resize_nearest(img, h, w):
    """cv2.resize(INTER_NEAREST): source index floor(dst * src / dst_size)."""
    ys = np.minimum((np.arange(h) * (img.shape[0] / h)).astype(np.int64), img.shape[0] - 1)
    xs = np.minimum((np.arange(w) * (img.shape[1] / w)).astype(np.int64), img.shape[1] - 1)
    return img[ys][:, xs]


def save_img(img, img_path, mode='RGB', scale=None):
    """cv2.imwrite of a BGR(A) / gray image (utils.py:92-96), through PIL when OpenCV is absent."""
    if scale:
        img = _resize_nearest(img, int(round(img.shape[0] * scale)), int(round(img.shape[1] * scale)))
    if cv2_available:
        cv2.imwrite(img_path, img)
        return
    from PIL import Image
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 3:
        a = a[:, :, ::-1]
    elif a.ndim == 3 and a.shape[2] == 4:
        a = a[:, :, [2, 1, 0, 3]]
    elif a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    Image.fromarray(np.ascontiguousarray(a)).save(img_path)


def merge_imgs(img_list):
    """Images side by side, the smaller ones enlarged (nearest) to the largest height / width (utils.py:99-124)."""
    if isinstance(img_list, np.ndarray):
        return img_list
    if not isinstance(img_list, list):
        raise NotImplementedError('To merge images img_list should be a list of cv2 images.')
    img_h = max(im.shape[0] for im in img_list)
    img_v = max(im.shape[1] for im in img_list)
    return np.concatenate([im if im.shape[:2] == (img_h, img_v) else _resize_nearest(im, img_h, img_v) for im in img_list], axis=1)


def save_img_comp(img_list, img_path, mode='RGB'):
    save_img(img=merge_imgs(img_list), img_path=img_path, mode=mode)


def modcrop(img_in, scale):
    """utils.py:250-264."""
    img = np.copy(img_in)
    if img.ndim not in (2, 3):
        raise ValueError('Wrong img ndim: [{:d}].'.format(img.ndim))
    H, W = img.shape[:2]
    return img[:H - H % scale, :W - W % scale]


def linear_resize(img, st=256, device='cuda'):
    """utils.py:267-276: enlarge to the next multiple of `st` in linear light (srgb2linear -> bicubic -> linear2srgb), on the GPU
    (csrc/colorfix.hip; the bicubic follows OpenCV's INTER_CUBIC formulas -- parity with OpenCV itself is unpinned, as for color_fix)."""
    h, w = img.shape[0:2]
    if h % st == 0 and w % st == 0:
        return img
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError('linear_resize: expected a uint8 HWC numpy image')
    oh, ow = -(-h // st) * st, -(-w // st) * st
    Cc = img.shape[2]
    d_in = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    out = torch.empty((oh, ow, Cc), dtype=torch.uint8, device=d_in.device)
    ws = torch.empty(h * w * Cc * 4, dtype=torch.uint8, device=d_in.device)
    with _on(out):
        L.check(L.lib.innfer_linear_resize(d_in.data_ptr(), h, w, Cc, out.data_ptr(), oh, ow, ws.data_ptr(), ws.numel(), _stream(out)))
    return out.cpu().numpy()


COLOR_FIX_MODES = tuple(L.COLOR_FIX_MODES)


def _cubic_taps_np(dst_size, src_size):
    """cubic_taps of csrc/colorfix.hip for every destination index of an axis: the four clamped source indices and the four float32 weights
    (A = -0.75, src = (dst + 0.5) * (src_size / dst_size) - 0.5)."""
    f32 = np.float32
    A, one = f32(-0.75), f32(1)
    f = (np.arange(dst_size, dtype=np.float32) + f32(0.5)) * (f32(src_size) / f32(dst_size)) - f32(0.5)
    fl = np.floor(f)
    t = f - fl
    w0 = ((A * (t + one) - f32(5) * A) * (t + one) + f32(8) * A) * (t + one) - f32(4) * A
    w1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    w2 = ((A + f32(2)) * (one - t) - (A + f32(3))) * (one - t) * (one - t) + one
    w3 = one - w0 - w1 - w2
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, src_size - 1)
    return idx, np.stack([w0, w1, w2, w3], 1)


def _cubic_enlarge_np(x, oh, ow):
    """cubic_sample of csrc/colorfix.hip for every pixel of the oh x ow result: per source row r = 0 + s0 w0 + s1 w1 + s2 w2 + s3 w3 along x, then
    acc = acc + r * wy[j] over the four rows; float32 HWC."""
    ix, wx = _cubic_taps_np(ow, x.shape[1])
    iy, wy = _cubic_taps_np(oh, x.shape[0])
    rows = np.zeros((x.shape[0], ow, x.shape[2]), np.float32)
    for k in range(4):
        rows = rows + x[:, ix[:, k]] * wx[:, k].reshape(1, ow, 1)
    acc = np.zeros((oh, ow, x.shape[2]), np.float32)
    for k in range(4):
        acc = acc + rows[iy[:, k]] * wy[:, k].reshape(oh, 1, 1)
    return acc


def _atrous_np(x, levels=5):
    """`levels` a-trous levels of the [0.25, 0.5, 0.25] filter, dilation 2^i: along x, then along y, replicate border, float32."""
    f32 = np.float32
    for i in range(levels):
        r = 1 << i
        for axis in (1, 0):
            n = x.shape[axis]
            p = np.arange(n)
            lo, hi = np.take(x, np.clip(p - r, 0, n - 1), axis=axis), np.take(x, np.clip(p + r, 0, n - 1), axis=axis)
            x = x * f32(0.5) + (lo + hi) * f32(0.25)
    return x


def _adain_stats_np(img):
    """Per channel (mean, unbiased variance) in float64 from the exact integer sums of the uint8 image."""
    n = img.shape[0] * img.shape[1]
    x = img.reshape(n, img.shape[2]).astype(np.int64)
    m = x.sum(0).astype(np.float64) / np.float64(n)
    q = (x * x).sum(0).astype(np.float64) / np.float64(n)
    var = np.maximum(q - m * m, 0.0) * (np.float64(n) / np.float64(n - 1)) if n > 1 else np.zeros_like(m)
    return m, var


def color_fix_np(imgA, imgB, mode):
    """The contract of the colour fixes that are not the reference's (`-cf_mode wavelet | adain`), in numpy; innfer_color_fix_mode computes the same
    codes.  imgA: the LR image, imgB: the SR image, uint8 HWC with one C in 1 .. 4, of equal sizes or with hA < hB and wA < wB.  Channels are
    independent; alpha is one more channel.
    'wavelet' (StableSR's wavelet reconstruction: SR's high band on LR's low band, as one decomposition of the difference), float32, code units:
    d = up - f32(imgB), up = f32(imgA) or its cubic enlargement to B's size (_cubic_enlarge_np: the arithmetic of csrc/colorfix.hip's cubic_sample);
    five a-trous levels of d (_atrous_np); clamp(floor(f32(imgB) + B5(d) + 0.5), 0, 255).
    'adain': per channel, from the exact integer sums, in float64: m = S1 / n, q = S2 / n, var = max(q - m m, 0) n / (n - 1) (0 for n = 1),
    eps = 1e-5 * 255 * 255, g = sqrt(varA + eps) / sqrt(varB + eps), o = mA - mB g; clamp(floor(f32(imgB) * f32(g) + f32(o) + 0.5), 0, 255) with the
    product and the sum each rounded to float32.  LR's statistics are those of the LR image itself.
    'lowfreq' is color_fix itself (the reference's fix) and is not restated here."""
    for im in (imgA, imgB):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3:
            raise TypeError('color_fix_np: expected uint8 HWC numpy images')
    if mode not in ('wavelet', 'adain'):
        raise ValueError(f"color_fix_np: mode must be 'wavelet' or 'adain', got {mode!r}")
    if imgA.shape[2] != imgB.shape[2] or not 1 <= imgA.shape[2] <= 4:
        raise ValueError('color_fix_np: both images need the same channel count in 1 .. 4')
    (hA, wA), (hB, wB) = imgA.shape[:2], imgB.shape[:2]
    scaling = hA < hB and wA < wB
    if not scaling and (hA, wA) != (hB, wB) or min(hA, wA, hB, wB) < 1:
        raise ValueError(f'color_fix_np: images of {hA}x{wA} and {hB}x{wB} cannot be subtracted')
    f32 = np.float32
    b = imgB.astype(np.float32)
    if mode == 'wavelet':
        up = _cubic_enlarge_np(imgA.astype(np.float32), hB, wB) if scaling else imgA.astype(np.float32)
        v = b + _atrous_np(up - b)
    else:
        (mA, vA), (mB, vB) = _adain_stats_np(imgA), _adain_stats_np(imgB)
        eps = np.float64(1e-5 * 255 * 255)
        g = np.sqrt(vA + eps) / np.sqrt(vB + eps)
        o = mA - mB * g
        v = b * g.astype(np.float32) + o.astype(np.float32)
    return np.clip(np.floor(v + f32(0.5)), 0, 255).astype(np.uint8)


def color_fix(imgA, imgB, device='cuda', mode='lowfreq', out=None):
    """`-cf` (utils.py:278-315): add the low-frequency LR - SR difference (linear light) back to the SR
    image.  imgA (LR) and imgB (SR) are uint8 HWC numpy images like the reference's; both cross PCIe as
    uint8, everything else runs in libinnfer_amd.so (csrc/colorfix.hip); returns a uint8 HWC numpy image.
    The reference's two OpenCV calls (bicubic resize, 3x3 Gaussian) follow OpenCV's published float32
    algorithms -- OpenCV itself is not available here to compare with.
    mode: 'lowfreq' is that fix; 'wavelet' and 'adain' are color_fix_np's (`-cf_mode`), to the code.
    Two cuda uint8 tensors stay on the GPU: the result is a cuda tensor (`out` when given: contiguous, of imgB's shape), launched on the current stream."""
    code = L.color_fix_mode(mode)
    dev_in = torch.is_tensor(imgA) and torch.is_tensor(imgB)
    if dev_in:
        for im in (imgA, imgB):
            if im.dtype != torch.uint8 or im.dim() != 3:
                raise TypeError('color_fix: expected uint8 HWC tensors')
            _need_cuda(im, 'color_fix')
        if imgA.device != imgB.device:
            raise ValueError('color_fix: the two images are on different devices')
    else:
        for im in (imgA, imgB):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3:
                raise TypeError('color_fix: expected uint8 HWC numpy images')
    if imgA.shape[2] != imgB.shape[2]:
        raise ValueError('color_fix: channel counts differ')
    hA, wA, Cc = imgA.shape
    hB, wB, _ = imgB.shape
    if dev_in:
        d_a, d_b = imgA.contiguous(), imgB.contiguous()
    else:
        d_a = torch.from_numpy(np.ascontiguousarray(imgA)).to(device)
        d_b = torch.from_numpy(np.ascontiguousarray(imgB)).to(device)
    if out is None:
        out = torch.empty((hB, wB, Cc), dtype=torch.uint8, device=d_a.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != (hB, wB, Cc) or out.dtype != torch.uint8 or out.device != d_a.device or not out.is_contiguous():
        raise ValueError(f'color_fix: out must be a contiguous uint8 tensor of shape {(hB, wB, Cc)} on {d_a.device}')
    elif out.data_ptr() == d_b.data_ptr() or out.data_ptr() == d_a.data_ptr():
        raise ValueError('color_fix: out must not be one of the two images (neighbouring pixels are read after the first are written)')
    if code == 0:                                               # the reference's fix: the call it has always been
        ws = torch.empty(L.lib.innfer_color_fix_workspace_bytes(hA, wA, hB, wB, Cc), dtype=torch.uint8, device=d_a.device)
        with _on(out):
            L.check(L.lib.innfer_color_fix(d_a.data_ptr(), hA, wA, d_b.data_ptr(), hB, wB, Cc, out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(out)))
    else:
        ws = torch.empty(max(1, L.lib.innfer_color_fix_mode_workspace_bytes(code, hA, wA, hB, wB, Cc)), dtype=torch.uint8, device=d_a.device)
        with _on(out):
            L.check(L.lib.innfer_color_fix_mode(code, d_a.data_ptr(), hA, wA, d_b.data_ptr(), hB, wB, Cc, out.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream(out)))
    return out if dev_in else out.cpu().numpy()


def guided_filter(x, y, x_HR=None, ks=None, r=None, eps=1e-2, box_kernel=None, mode='regular', conv_a=None):
    """guided_filter (utils.py:548-626): 'regular' mode (what run.py:427-429 applies after the WBC UNet with r=1) and 'fast' mode (A, b of the
    low-resolution pair enlarged bilinearly to the high-resolution guidance x_HR), any odd window ks = 2 r + 1 (box means, reflect padding);
    x guidance, y input, [B,C,H,W] GPU tensors of one dtype.  Runs in libinnfer_amd.so (csrc/wbcunet.hip: one fused pass per stage).  The remaining
    forms -- 'conv' mode (the caller's nn.Sequential `conv_a` computes A from cat(cov_xy, var_x)), a precomputed box_kernel tensor, even window
    sizes -- follow the reference's formula step by step on the HIP filter2D (its box means) with the caller's module in between."""
    if mode not in ('regular', 'fast', 'conv'):
        raise NotImplementedError("guided_filter: modes 'regular', 'fast' and 'conv'")
    if not isinstance(box_kernel, torch.Tensor):
        if not ks:
            if not r:
                raise ValueError("Either kernel size (ks) or radius (r) for the window are required.")
            ks = 2 * r + 1
    if mode == 'conv' or isinstance(box_kernel, torch.Tensor) or int(ks) != ks or int(ks) % 2 == 0:
        return _guided_filter_stepwise(x, y, x_HR, box_kernel if isinstance(box_kernel, torch.Tensor) else get_box_kernel(kernel_size=ks), eps, mode, conv_a)
    if mode == 'fast' and not isinstance(x_HR, torch.Tensor):
        raise ValueError("guided_filter: mode 'fast' needs the high-resolution guidance x_HR")
    _need_cuda(x, 'guided_filter')
    if x.shape != y.shape or x.dtype != y.dtype or x.dim() != 4:
        raise ValueError('guided_filter: x and y must be [B,C,H,W] tensors of one shape and dtype')
    x, y = x.contiguous(), y.contiguous()
    B, Cc, H, W = x.shape
    hr = None
    if mode == 'fast':
        hr = x_HR.contiguous()
        if hr.dim() != 4 or hr.shape[:2] != x.shape[:2] or hr.dtype != x.dtype or hr.device != x.device:
            raise ValueError('guided_filter: x_HR must be a [B,C,Hh,Wh] tensor with the batch, channels, dtype and device of x')
    out = torch.empty_like(hr if hr is not None else x)
    ws = torch.empty(L.lib.innfer_guided_filter_workspace_bytes(B, Cc, H, W), dtype=torch.uint8, device=x.device)
    with _on(x):
        L.check(L.lib.innfer_guided_filter_ex(x.data_ptr(), y.data_ptr(), _dt(x), B, Cc, H, W, int(ks), float(eps),
                                              hr.data_ptr() if hr is not None else None, hr.shape[2] if hr is not None else 0,
                                              hr.shape[3] if hr is not None else 0, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)))
    return out


def _guided_filter_stepwise(x, y, x_HR, box_kernel, eps, mode, conv_a):
    """utils.py:590-626 step by step: box means by the HIP filter2D, the products / quotients as tensor expressions, `conv_a` the caller's module."""
    import torch.nn.functional as F
    _need_cuda(x, 'guided_filter')
    if mode in ('fast', 'conv') and not isinstance(x_HR, torch.Tensor):
        raise ValueError(f"guided_filter: mode '{mode}' needs the high-resolution guidance x_HR")
    if mode == 'conv' and conv_a is None:
        raise ValueError("guided_filter: mode 'conv' needs conv_a")
    box_kernel = box_kernel.to(x.device)
    N = filter2D(torch.ones((1, 1, x.shape[-2], x.shape[-1]), device=x.device, dtype=x.dtype), box_kernel)
    mean_x = filter2D(x, box_kernel) / N
    mean_y = filter2D(y, box_kernel) / N
    cov_xy = (filter2D(x * y, box_kernel) / N) - mean_x * mean_y
    var_x = (filter2D(x * x, box_kernel) / N) - mean_x * mean_x
    A = conv_a(torch.cat([cov_xy, var_x], dim=1)) if mode == 'conv' else cov_xy / (var_x + eps)
    b = mean_y - A * mean_x
    if mode in ('fast', 'conv'):
        size = (x_HR.shape[-2], x_HR.shape[-1])
        return F.interpolate(A, size, mode='bilinear', align_corners=True) * x_HR + F.interpolate(b, size, mode='bilinear', align_corners=True)
    return (filter2D(A, box_kernel) / N) * x + filter2D(b, box_kernel) / N


# --------------------------------------------------------------- small helpers of the reference's utils (host math / elementwise plumbing)
def denorm(x, min_max=(-1.0, 1.0)):
    """[min, max] -> [0, 1], clamped (utils.py:136-150).  The image path applies it inside tensor2np / the uint8 epilogue; this is the free function."""
    out = (x - min_max[0]) / (min_max[1] - min_max[0])
    if isinstance(x, torch.Tensor):
        return out.clamp(0, 1)
    if isinstance(x, np.ndarray):
        return np.clip(out, 0, 1)
    raise TypeError("Got unexpected object type, expected torch.Tensor or np.ndarray")


def norm(x):
    """[0, 1] -> [-1, 1], clamped (utils.py:152-161)."""
    out = (x - 0.5) * 2.0
    if isinstance(x, torch.Tensor):
        return out.clamp(-1, 1)
    if isinstance(x, np.ndarray):
        return np.clip(out, -1, 1)
    raise TypeError("Got unexpected object type, expected torch.Tensor or np.ndarray")


def filter2D(x, kernel, border_type='reflect', dim=2, normalized=False):
    """Every channel of x [B,C,H,W] convolved (cross-correlated) with one [1,kH,kW] kernel behind F.pad(x, compute_padding((kH, kW)), border_type):
    the output keeps x's shape and dtype (utils.py:484-535).  HIP kernel (csrc/wbcunet.hip k_filter2d); dim 2 only."""
    borders = ['constant', 'reflect', 'replicate', 'circular']
    if border_type not in borders:
        raise ValueError("Invalid border_type, we expect the following: {0}.Got: {1}".format(borders, border_type))
    if dim != 2:
        raise NotImplementedError("filter2D: 2-D tensors are built (the reference's only use)")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError('expected a 4D [B,C,H,W] tensor')
    if not x.is_cuda:
        raise RuntimeError('innfer_amd runs filter2D on an MI355X only: there is no CPU path')
    k = kernel.unsqueeze(0).to(x.device).to(x.dtype)
    if normalized:
        k = normalize_kernel2d(k)
    kH, kW = int(k.shape[-2]), int(k.shape[-1])
    pad = compute_padding((kH, kW))                                   # (left, right, top, bottom)
    if pad[0] + pad[1] != kW - 1 or pad[2] + pad[3] != kH - 1:
        raise NotImplementedError("filter2D: this kernel shape changes the output size in the reference (mixed even / odd sides)")
    x = x.contiguous() if x.dtype in (torch.float16, torch.float32) else x.float().contiguous()
    kd = k.reshape(kH, kW).float().contiguous()
    out = torch.empty_like(x)
    B, Cc, H, W = x.shape
    with _on(x):
        L.check(L.lib.innfer_filter2d(x.data_ptr(), _dt(x), B * Cc, H, W, kd.data_ptr(), kH, kW, int(pad[0]), int(pad[2]), borders.index(border_type),
                                      out.data_ptr(), _stream(x)))
    return out


def get_box_kernel(kernel_size=5, dim=2):
    """The mean filter of guided_filter as a tensor (utils.py:538-546): ones / (kx * ky)."""
    if isinstance(kernel_size, (int, float)):
        kernel_size = [kernel_size] * dim
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    return torch.full((kx, ky), 1.0 / (float(kx) * float(ky)), dtype=torch.float32)


def normalize_kernel2d(x):
    """L1-normalise the last two axes of a kernel (utils.py:448-454)."""
    if x.dim() < 2:
        raise TypeError("input should be at least 2D tensor. Got {}".format(x.size()))
    return x / x.abs().sum(dim=(-1, -2), keepdim=True)


def compute_padding(kernel_size):
    """Padding that keeps the size under a kernel (utils.py:457-481): k // 2 for an int; for a tuple / list one (before, after) pair per axis,
    last axis first, the 'before' side one less for even kernels."""
    if isinstance(kernel_size, int):
        return kernel_size // 2
    ks = list(kernel_size)
    half = [k // 2 for k in ks]
    out = []
    for i in range(len(ks)):
        after = half[-(i + 1)]
        out += [after - 1 if ks[i] % 2 == 0 else after, after]
    return out


# --------------------------------------------------------------- key converters
_NEW2OLD_FIXED = (('conv_first', 'model.0'), ('trunk_conv', 'model.1.sub.23'), ('upconv1', 'model.3'),
                  ('upconv2', 'model.6'), ('HRconv', 'model.8'), ('conv_last', 'model.10'))


def mod2normal(state_dict):
    """New-arch ESRGAN keys (conv_first / RRDB_trunk.N.RDBk.convj / trunk_conv /
    upconv1,2 / HRconv / conv_last) -> old-arch keys (utils.py:666-698).  Like the
    reference this assumes the 23-block 4x layout ('model.1.sub.23', 'model.3' ...)."""
    if 'conv_first.weight' not in state_dict:
        return state_dict
    print('Converting and loading a modified RRDB model to normal RRDB')
    out = {}
    for new, old in _NEW2OLD_FIXED[:1]:
        for p in ('weight', 'bias'):
            out[f'{old}.{p}'] = state_dict[f'{new}.{p}']
    for k, v in state_dict.items():
        if 'RDB' in k:
            k2 = k.replace('RRDB_trunk.', 'model.1.sub.')
            if '.weight' in k:
                k2 = k2.replace('.weight', '.0.weight')
            elif '.bias' in k:
                k2 = k2.replace('.bias', '.0.bias')
            out[k2] = v
    for new, old in _NEW2OLD_FIXED[1:]:
        for p in ('weight', 'bias'):
            out[f'{old}.{p}'] = state_dict[f'{new}.{p}']
    return out


def normal2mod(state_dict):
    """Old-arch ESRGAN keys -> new-arch keys (utils.py:629-663), the inverse of mod2normal; like the reference it assumes the 23-block 4x layout."""
    if 'model.0.weight' not in state_dict:
        return state_dict
    print('Converting and loading an RRDB model to modified RRDB')
    out = {}
    for new, old in _NEW2OLD_FIXED[:1]:
        for p in ('weight', 'bias'):
            out[f'{new}.{p}'] = state_dict[f'{old}.{p}']
    for k, v in state_dict.items():
        if 'RDB' in k:
            k2 = k.replace('model.1.sub.', 'RRDB_trunk.')
            if '.0.weight' in k:
                k2 = k2.replace('.0.weight', '.weight')
            elif '.0.bias' in k:
                k2 = k2.replace('.0.bias', '.bias')
            out[k2] = v
    for new, old in _NEW2OLD_FIXED[1:]:
        for p in ('weight', 'bias'):
            out[f'{new}.{p}'] = state_dict[f'{old}.{p}']
    return out


def unwrap_params(state_dict):
    """The state dict inside a BasicSR / Real-ESRGAN checkpoint: those files hold {'params_ema': {...}} and / or {'params': {...}}; the EMA weights are
    the ones BasicSR's own loaders prefer.  Anything else is returned as it is."""
    if isinstance(state_dict, dict):
        for name in ('params_ema', 'params'):
            if isinstance(state_dict.get(name), dict):
                return state_dict[name]
    return state_dict


def realesrgan2normal(state_dict):
    """BasicSR RRDBNet keys (conv_first / body.N.rdbM.convK / conv_body / conv_up1,2 / conv_hr / conv_last) -> old-arch keys, for any number of blocks
    (architectures.keys.realesrgan_key_map).  conv_first keeps its in_nc * r^2 input channels: the old-arch graph then takes pixel_unshuffle(x, r)."""
    from ..architectures.keys import realesrgan_key_map
    nb = 1 + max(int(k.split('.')[1]) for k in state_dict if k.startswith('body.'))
    out = {}
    for new, old in realesrgan_key_map(nb).items():
        for p in ('weight', 'bias'):
            out[f'{old}.{p}'] = state_dict[f'{new}.{p}']
    return out


def swa2normal(state_dict):
    """Unwrap a torch.optim.swa_utils.AveragedModel checkpoint: keep only
    'module.module.*' entries, stripped of that prefix (utils.py:701-720)."""
    if 'n_averaged' not in state_dict:
        return state_dict
    print('Attempting to convert a SWA model to a regular model\n')
    out = {}
    for k, v in state_dict.items():
        if 'n_averaged' in k:
            print('n_averaged: {}'.format(v))
        elif 'module.module.' in k:
            out[k.replace('module.module.', '')] = v
    return out
