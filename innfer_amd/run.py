"""Mirror of the reference's `Model` wrapper (run.py:23-225): .pth loading with
architecture / scale inference, and `Model.__call__` -> chop_forward.

Differences that are the point of this build:
  * the network forward, tile extraction and blend run in HIP (libinnfer_amd.so);
  * chop tiles are pushed through the network in BATCHES (the reference loops
    batch-1 and calls empty_cache() per tile, run.py:186-197); per-tile results
    are identical because tiles are independent.  tile_batch=None sizes the
    batches from the engine's workspace and the free memory (parallel.engine_tile_cap:
    <= 272 tiles per launch; an allocator OOM halves the batch and goes on);
  * with torch.distributed initialised, tiles can be sharded over ranks and
    gathered on rank 0 (parallel.py).
There is no CPU execution path: device must be a GPU.
"""
import torch

from .architectures import get_network
from .utils.defaults import get_network_G_config
from .utils.utils import extract_patches_2d, mod2normal, recompose_tensor, swa2normal, unwrap_params

# families the HIP engine implements; the other branches of the reference's key
# sniffing are recognised and refused explicitly
_SNIFF = (
    ('SCPA_trunk.0.conv1_a.weight', 'pan'),
    ('model.1.sub.0.res.0.weight', 'srgan'),
    ('body.0.rdb1.conv1.weight', 'realesrgan'),      # BasicSR's RRDBNet (with conv_first.weight): ahead of the new-arch probe, which shares conv_first
    ('body.0.weight', 'compact'),                    # BasicSR's SRVGGNetCompact: `body` is a ModuleList whose entry 0 is a conv (no body.0.rdb1.*)
    ('conv_1.sk.weight', 'span'),                    # SPAN (with conv_cat.weight): a full checkpoint ..
    ('conv_1.eval_conv.weight', 'span'),             # .. or a `deploy` one, which carries only the collapsed convs
    ('feats.0.weight', 'realplksr'),                 # RealPLKSR (with feats.1.channel_mixer.0.weight)
    ('layers.0.residual_group.blocks.0.norm1.weight', 'swinir'),      # SwinIR and what builds on its skeleton (with conv_first.weight): ahead of the new-arch probe
    ('before_RG.1.weight', 'dat'),                   # DAT (with conv_first.weight and block 0's complete key set, _DAT_KEYS): ahead of the new-arch probe
    ('layers.0.swin1.norm1.weight', 'drct'),         # DRCT (with conv_first.weight and dense group 0's complete key set, _DRCT_KEYS): ahead of the new-arch probe
    ('conv_first.weight', 'mesrgan'),
    ('model.0.weight', 'esrgan'),
    ('CFEM.0.weight', 'ppon'),
    ('conv_9.weight', 'wbcunet'),
)


def infer_from_state_dict(state_dict, scale=None, in_nc=3, out_nc=3):
    """Architecture, scale and hyper-parameters from a checkpoint's key names and
    shapes -- host logic of Model.load_model / infer_params (run.py:44-72,103-165).
    Returns dict(arch, scale, in_nc, out_nc, nf, nb, plus, net_params, state_dict)
    where state_dict has been SWA-unwrapped / converted to old-arch keys."""
    state_dict = unwrap_params(state_dict)
    if 'n_averaged' in state_dict:
        state_dict = swa2normal(state_dict)
    for probe, arch in _SNIFF:
        if probe in state_dict and (arch != 'realesrgan' or 'conv_first.weight' in state_dict) and (arch != 'span' or 'conv_cat.weight' in state_dict) and \
                (arch != 'realplksr' or 'feats.1.channel_mixer.0.weight' in state_dict) and (arch != 'swinir' or 'conv_first.weight' in state_dict) and \
                (arch != 'dat' or all(k in state_dict for k in _DAT_KEYS)) and (arch != 'drct' or all(k in state_dict for k in _DRCT_KEYS)):
            break
    else:
        raise Exception("Could not infer model parameters.")
    if arch == 'mesrgan':                    # new-arch checkpoints run as old-arch (run.py:57-61)
        state_dict = mod2normal(state_dict)
        arch = 'esrgan'
    if arch == 'realesrgan':
        return _infer_realesrgan(state_dict, in_nc)
    if arch == 'compact':
        return _infer_compact(state_dict)
    if arch == 'span':
        return _infer_span(state_dict)
    if arch == 'realplksr':
        return _infer_realplksr(state_dict)
    if arch == 'swinir':
        hat = _infer_hat(state_dict)         # (a complete HAT key set; anything less goes on to SwinIR's sniffing and its refusals)
        if hat is not None:
            return hat
        s2 = _infer_swin2sr(state_dict)      # (likewise: block 0's complete Swin2SR key set)
        return s2 if s2 is not None else _infer_swinir(state_dict)
    if arch == 'dat':
        return _infer_dat(state_dict)
    if arch == 'drct':
        return _infer_drct(state_dict)
    if arch == 'pan':
        return _infer_pan(state_dict, scale, in_nc, out_nc)
    if arch == 'ppon':
        return _infer_ppon(state_dict, scale, in_nc, out_nc)
    if arch == 'wbcunet':                    # run.py:150-156: scale 1, mode 'pt', nf from the first conv
        cfg = {'type': 'wbcunet', 'mode': 'pt', 'nf': int(state_dict['conv.weight'].shape[0])}
        return dict(arch='wbcunet', scale=1, in_nc=3, out_nc=3, nf=cfg['nf'], nb=4, plus=False, state_dict=state_dict,
                    net_params=get_network_G_config(cfg, 1))
    if arch not in ('esrgan', 'srgan'):
        raise NotImplementedError(f"'{arch}' checkpoints are recognised but not on the HIP path yet")
    top = {}                                 # N -> out channels of 'model.N.weight|bias'
    nb = None
    n_2x = 0
    for key, val in state_dict.items():
        parts = key.split('.')
        if len(parts) == 5 and parts[2] == 'sub':
            nb = int(parts[3])               # the trunk conv sits right after the last block
        elif len(parts) == 3:
            n = int(parts[1])
            top.setdefault(n, val.shape[0])
            if n > 6 and parts[0] == 'model' and parts[2] == 'weight':
                n_2x += 1                    # every top-level conv past index 6 = one 2x stage
    w0 = state_dict['model.0.weight']
    info = dict(arch=arch, scale=2 ** n_2x, in_nc=int(w0.shape[1]), out_nc=int(top[max(top)]),
                nf=int(w0.shape[0]), nb=nb, plus=False, state_dict=state_dict)
    cfg = {'type': arch, 'in_nc': info['in_nc'], 'out_nc': info['out_nc'], 'nf': info['nf'], 'nb': nb}
    if arch == 'esrgan':
        info['plus'] = any('conv1x1' in k for k in state_dict)
        cfg['plus'] = info['plus']
    info['net_params'] = get_network_G_config(cfg, info['scale'])
    return info


def _infer_realesrgan(state_dict, in_nc=3):
    """BasicSR RRDBNet checkpoints (Real-ESRGAN x4plus, x4plus_anime_6B, x2plus, ...): everything is read off the keys and shapes.  The state dict keeps
    BasicSR's keys -- the RealESRGANNet shell registers its parameters under them."""
    blocks = {int(k.split('.')[1]) for k in state_dict if k.startswith('body.')}
    nb = max(blocks) + 1
    if blocks != set(range(nb)):
        raise Exception("Could not infer model parameters.")
    w0 = state_dict['conv_first.weight']
    nf, cin = int(w0.shape[0]), int(w0.shape[1])
    gc = int(state_dict['body.0.rdb1.conv1.weight'].shape[0])
    if gc != 32:
        raise NotImplementedError(f'BasicSR RRDBNet checkpoint with num_grow_ch={gc}: only 32 is built on the HIP path')
    out_nc = int(state_dict['conv_last.weight'].shape[0])
    # conv_first takes in_nc * r^2 channels behind pixel_unshuffle(r): 3, 12 or 48 for RGB.  A count that is not in_nc times 1, 4 or 16 is a plain 4x model of that many channels.
    r = {1: 1, 4: 2, 16: 4}.get(cin // in_nc if in_nc and cin % in_nc == 0 else 0)
    if r is None:
        r, in_nc = 1, cin
    scale = 4 // r
    cfg = {'type': 'realesrgan', 'in_nc': in_nc, 'out_nc': out_nc, 'nf': nf, 'nb': nb, 'gc': gc, 'scale': scale}
    return dict(arch='realesrgan', scale=scale, in_nc=in_nc, out_nc=out_nc, nf=nf, nb=nb, plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, scale))


def _infer_compact(state_dict):
    """BasicSR SRVGGNetCompact checkpoints (realesr-animevideov3, realesr-general-x4v3, "compact" community models): num_feat, num_in_ch and num_conv are read
    off the keys, upscale = sqrt(last conv's channels / num_in_ch).  ReLU and LeakyReLU nets carry no activation parameters and cannot be told apart from the
    keys: only PReLU checkpoints are inferred."""
    import math
    w0 = state_dict['body.0.weight']
    if w0.dim() != 4 or any(k.startswith('body.0.rdb') for k in state_dict):
        raise Exception("Could not infer model parameters.")
    convs = sorted(int(k.split('.')[1]) for k, v in state_dict.items() if k.startswith('body.') and k.endswith('.weight') and v.dim() == 4)
    last = convs[-1]
    if len(convs) < 2 or convs != list(range(0, last + 1, 2)):
        raise Exception("Could not infer model parameters.")
    nf, in_nc = int(w0.shape[0]), int(w0.shape[1])
    num_conv = len(convs) - 2
    k_last = int(state_dict[f'body.{last}.weight'].shape[0])
    up = math.isqrt(k_last // in_nc) if k_last % in_nc == 0 else 0
    if up * up * in_nc != k_last:
        raise NotImplementedError(f'SRVGGNetCompact checkpoint: the last conv has {k_last} channels, not num_in_ch ({in_nc}) times a square '
                                  '(num_out_ch != num_in_ch is not built on the HIP path)')
    a1 = state_dict.get('body.1.weight')
    if a1 is None or a1.dim() != 1 or any(f'body.{i + 1}.weight' not in state_dict for i in convs[:-1]):
        raise NotImplementedError("SRVGGNetCompact checkpoint without PReLU weights: ReLU and LeakyReLU(0.1) nets cannot be told apart from the keys -- "
                                  "build SRVGGNetCompact(act_type=...) and load the state dict instead of arch='infer'")
    cfg = {'type': 'compact', 'in_nc': in_nc, 'out_nc': in_nc, 'nf': nf, 'nb': num_conv, 'scale': up, 'act_type': 'prelu'}
    return dict(arch='compact', scale=up, in_nc=in_nc, out_nc=in_nc, nf=nf, nb=num_conv, plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


def _infer_span(state_dict):
    """SPAN checkpoints: feature_channels from conv_cat, num_in_ch from conv_1, upscale = sqrt(upsampler.0's channels / num_in_ch); `no_norm` marks the
    norm=False variant of the community training framework, absent `sk` keys a `deploy` checkpoint (only the collapsed eval_conv per Conv3XC)."""
    import math
    deploy = 'conv_1.sk.weight' not in state_dict
    w1 = state_dict['conv_1.eval_conv.weight' if deploy else 'conv_1.sk.weight']
    wc = state_dict['conv_cat.weight']
    if 'upsampler.0.weight' not in state_dict or wc.dim() != 4 or int(wc.shape[1]) != 4 * int(wc.shape[0]):
        raise Exception("Could not infer model parameters.")
    f, in_nc = int(wc.shape[0]), int(w1.shape[1])
    k_up = int(state_dict['upsampler.0.weight'].shape[0])
    up = math.isqrt(k_up // in_nc) if k_up % in_nc == 0 else 0
    if up * up * in_nc != k_up:
        raise NotImplementedError(f'SPAN checkpoint: upsampler.0 has {k_up} channels, not num_in_ch ({in_nc}) times a square '
                                  '(num_out_ch != num_in_ch is not built on the HIP path)')
    norm = 'no_norm' not in state_dict
    cfg = {'type': 'span', 'in_nc': in_nc, 'out_nc': in_nc, 'nf': f, 'scale': up, 'norm': norm, 'deploy': deploy}
    return dict(arch='span', scale=up, in_nc=in_nc, out_nc=in_nc, nf=f, nb=6, plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


def _infer_realplksr(state_dict):
    """RealPLKSR checkpoints: dim and in_ch from feats.0, n_blocks from the highest feats.<i>.channel_mixer.0, kernel_size and split_ratio from feats.1.lk.conv, use_ea
    from feats.1.attn.f.0, the scale = sqrt(last conv's channels / in_ch).  norm_groups is not in the keys: the published default, 4.  DySample checkpoints (to_img.*) and
    the original PLKSR (no GroupNorm: feats.1.norm.weight missing) are refused."""
    import math
    if any(k.startswith('to_img.') for k in state_dict):
        raise NotImplementedError('RealPLKSR checkpoint with a DySample upsampler (to_img.* keys): not built on the HIP path')
    if 'feats.1.norm.weight' not in state_dict:
        raise NotImplementedError('PLKSR checkpoint without feats.1.norm.weight (the original PLKSR, no GroupNorm): only RealPLKSR is built on the HIP path')
    w0 = state_dict['feats.0.weight']
    dim, in_nc = int(w0.shape[0]), int(w0.shape[1])
    n_blocks = 0
    while f'feats.{n_blocks + 1}.channel_mixer.0.weight' in state_dict:
        n_blocks += 1
    last = f'feats.{n_blocks + 2}.weight'
    if last not in state_dict or 'feats.1.lk.conv.weight' not in state_dict:
        raise Exception("Could not infer model parameters.")
    lk = state_dict['feats.1.lk.conv.weight']
    p, ks = int(lk.shape[0]), int(lk.shape[-1])
    k_last = int(state_dict[last].shape[0])
    up = math.isqrt(k_last // in_nc) if k_last % in_nc == 0 else 0
    if up * up * in_nc != k_last:
        raise NotImplementedError(f'RealPLKSR checkpoint: the last conv has {k_last} channels, not in_ch ({in_nc}) times a square '
                                  '(out_ch != in_ch is not built on the HIP path)')
    cfg = {'type': 'realplksr', 'in_nc': in_nc, 'out_nc': in_nc, 'nf': dim, 'nb': n_blocks, 'scale': up, 'kernel_size': ks, 'split_ratio': p / dim,
           'use_ea': 'feats.1.attn.f.0.weight' in state_dict}
    return dict(arch='realplksr', scale=up, in_nc=in_nc, out_nc=in_nc, nf=dim, nb=n_blocks, plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


def _infer_swinir(state_dict):
    """SwinIR checkpoints (the three super-resolution forms): embed_dim and in_chans from conv_first, depths by counting layers.<i>.residual_group.blocks.<j>, num_heads and
    the window from the relative position bias table ([(2 ws - 1)^2, nH]), mlp_ratio from mlp.fc1, '3conv' from layers.0.conv.0, the tail and the scale from the tail's keys.
    The buffers (attn.relative_position_index, attn_mask) are dropped from the state dict handed back: the engine rebuilds the index from its formula -- a stored index that
    differs is refused -- and computes the mask from the coordinates (the stored one is sized for img_size).  Swin2SR, HAT / DRCT, an absolute position embedding, a window
    other than 8, the denoising / JPEG forms (no upsampler) and checkpoints without patch_embed.norm or qkv biases are refused."""
    import math
    b0 = 'layers.0.residual_group.blocks.0.'
    if any(k.endswith('attn.logit_scale') for k in state_dict):
        raise NotImplementedError('Swin2SR checkpoint (attn.logit_scale: cosine attention, continuous position bias): not built on the HIP path')
    if any('overlap_attn' in k or 'conv_block' in k for k in state_dict):
        raise NotImplementedError('HAT / DRCT checkpoint (overlap_attn / conv_block keys): not built on the HIP path')
    if 'absolute_pos_embed' in state_dict:
        raise NotImplementedError('SwinIR checkpoint with absolute_pos_embed (ape=True): not built on the HIP path')
    if b0 + 'attn.relative_position_bias_table' not in state_dict or b0 + 'attn.qkv.weight' not in state_dict or b0 + 'mlp.fc1.weight' not in state_dict:
        raise Exception("Could not infer model parameters.")
    if 'patch_embed.norm.weight' not in state_dict:
        raise NotImplementedError('SwinIR checkpoint without patch_embed.norm (patch_norm=False): not built on the HIP path')
    if b0 + 'attn.qkv.bias' not in state_dict:
        raise NotImplementedError('SwinIR checkpoint without attn.qkv.bias (qkv_bias=False): not built on the HIP path')
    w0 = state_dict['conv_first.weight']
    C, in_nc = int(w0.shape[0]), int(w0.shape[1])
    depths = []
    while f'layers.{len(depths)}.residual_group.blocks.0.norm1.weight' in state_dict:
        i, j = len(depths), 0
        while f'layers.{i}.residual_group.blocks.{j}.norm1.weight' in state_dict:
            j += 1
        depths.append(j)
    table = state_dict[b0 + 'attn.relative_position_bias_table']
    nh, side = int(table.shape[1]), math.isqrt(int(table.shape[0]))
    ws = (side + 1) // 2
    if side * side != int(table.shape[0]) or 2 * ws - 1 != side:
        raise Exception("Could not infer model parameters.")
    if ws != 8:
        raise NotImplementedError(f'SwinIR checkpoint with window_size {ws}: only 8 x 8 windows are built on the HIP path')
    hidden = int(state_dict[b0 + 'mlp.fc1.weight'].shape[0])
    if 'conv_up1.weight' in state_dict:
        upsampler, up = 'nearest+conv', 4 if 'conv_up2.weight' in state_dict else 2
        out_nc = int(state_dict['conv_last.weight'].shape[0])
    elif 'conv_before_upsample.0.weight' in state_dict:
        upsampler, up = 'pixelshuffle', 1
        for k, v in state_dict.items():
            if k.startswith('upsample.') and k.endswith('.weight'):
                f = math.isqrt(int(v.shape[0]) // 64)
                if f * f * 64 != int(v.shape[0]):
                    raise Exception("Could not infer model parameters.")
                up *= f
        out_nc = int(state_dict['conv_last.weight'].shape[0])
    elif 'upsample.0.weight' in state_dict:
        upsampler = 'pixelshuffledirect'
        k_up = int(state_dict['upsample.0.weight'].shape[0])
        up = math.isqrt(k_up // in_nc) if k_up % in_nc == 0 else 0
        if up * up * in_nc != k_up:
            raise NotImplementedError(f'SwinIR checkpoint: upsample.0 has {k_up} channels, not in_chans ({in_nc}) times a square (more output than input channels is not built on the HIP path)')
        out_nc = in_nc
    else:
        raise NotImplementedError("SwinIR checkpoint without an upsampler (upsampler '': the denoising / JPEG models): only the super-resolution forms are built on the HIP path")
    if out_nc != in_nc:
        raise NotImplementedError(f'SwinIR checkpoint: conv_last has {out_nc} channels, conv_first takes {in_nc} (unequal channel counts are not built on the HIP path)')
    from .architectures.SwinIR_arch import relative_position_index
    want = relative_position_index(ws)
    for k in [k for k in state_dict if k.endswith('attn.relative_position_index')]:
        v = state_dict[k]
        if tuple(v.shape) != tuple(want.shape) or not bool((v.cpu().long() == want).all()):
            raise NotImplementedError(f'SwinIR checkpoint: {k} differs from (ri - rj + 7) * 15 + (ci - cj + 7), the index the engine builds its bias table with')
    state_dict = {k: v for k, v in state_dict.items() if not (k.endswith('attn.relative_position_index') or k.endswith('.attn_mask'))}
    cfg = {'type': 'swinir', 'in_nc': in_nc, 'nf': C, 'depths': depths, 'num_heads': [nh] * len(depths), 'window_size': ws, 'mlp_ratio': hidden / C, 'scale': up,
           'upsampler': upsampler, 'resi_connection': '3conv' if 'layers.0.conv.0.weight' in state_dict else '1conv'}
    return dict(arch='swinir', scale=up, in_nc=in_nc, out_nc=in_nc, nf=C, nb=sum(depths), plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


_SWIN2SR_KEYS = ('attn.logit_scale', 'attn.cpb_mlp.0.weight', 'attn.cpb_mlp.0.bias', 'attn.cpb_mlp.2.weight', 'attn.q_bias', 'attn.v_bias', 'attn.qkv.weight', 'norm1.weight',
                 'mlp.fc1.weight')


def _infer_swin2sr(state_dict):
    """Swin2SR checkpoints (classical, lightweight and real-world super-resolution, and fine-tunes), or None unless block 0 carries the complete key set (_SWIN2SR_KEYS) and
    neither attn.relative_position_bias_table nor attn.qkv.bias -- the caller then sniffs as before.  embed_dim and in_chans from conv_first, depths by counting blocks,
    num_heads from attn.logit_scale, the width of cpb_mlp from its first Linear, mlp_ratio from mlp.fc1, '3conv' from layers.0.conv.0, the tail and the scale as
    _infer_swinir.  There is no bias table to read the window from: it comes from attn.relative_coords_table ([1, 2 ws - 1, 2 ws - 1, 2]) or from
    attn.relative_position_index ([ws^2, ws^2]) when the checkpoint carries one, and is ASSUMED to be 8 otherwise.  A stored relative_coords_table is authoritative: it is
    handed on (coords_table) and feeds cpb_mlp in place of the formula; relative_position_index is rebuilt from its formula and a stored one that differs is refused;
    attn_mask is never read.  All three buffers are dropped from the state dict handed back.  The compressed-SR (pixelshuffle_aux), pixelshuffle_hf and JPEG / denoising
    forms, an absolute position embedding, another window, a checkpoint without patch_embed.norm or without q_bias / v_bias are refused."""
    import math
    import numpy as np
    b0 = 'layers.0.residual_group.blocks.0.'
    if b0 + 'attn.logit_scale' in state_dict and b0 + 'attn.cpb_mlp.0.weight' in state_dict and b0 + 'attn.qkv.weight' in state_dict and \
            b0 + 'attn.relative_position_bias_table' not in state_dict and b0 + 'attn.qkv.bias' not in state_dict and \
            (b0 + 'attn.q_bias' not in state_dict or b0 + 'attn.v_bias' not in state_dict):
        raise NotImplementedError('Swin2SR checkpoint without attn.q_bias / attn.v_bias (qkv_bias=False): not built on the HIP path')
    if any(b0 + k not in state_dict for k in _SWIN2SR_KEYS) or b0 + 'attn.relative_position_bias_table' in state_dict or b0 + 'attn.qkv.bias' in state_dict:
        return None
    if any(k.startswith(('conv_bicubic', 'conv_aux', 'conv_after_aux')) for k in state_dict):
        raise NotImplementedError('Swin2SR checkpoint with the pixelshuffle_aux tail (conv_bicubic / conv_aux / conv_after_aux: the compressed-SR release): not built on the HIP path')
    if any(k.startswith(('conv_first_hf', 'layers_hf', 'conv_after_body_hf', 'conv_before_upsample_hf', 'upsample_hf', 'conv_last_hf')) for k in state_dict):
        raise NotImplementedError('Swin2SR checkpoint with the pixelshuffle_hf tail (conv_first_hf / layers_hf): not built on the HIP path')
    if 'absolute_pos_embed' in state_dict:
        raise NotImplementedError('Swin2SR checkpoint with absolute_pos_embed (ape=True): not built on the HIP path')
    if 'patch_embed.norm.weight' not in state_dict:
        raise NotImplementedError('Swin2SR checkpoint without patch_embed.norm (patch_norm=False): not built on the HIP path')
    w0 = state_dict['conv_first.weight']
    C, in_nc = int(w0.shape[0]), int(w0.shape[1])
    depths = []
    while f'layers.{len(depths)}.residual_group.blocks.0.norm1.weight' in state_dict:
        i, j = len(depths), 0
        while f'layers.{i}.residual_group.blocks.{j}.norm1.weight' in state_dict:
            j += 1
        depths.append(j)
    nh = int(state_dict[b0 + 'attn.logit_scale'].shape[0])
    cpb = int(state_dict[b0 + 'attn.cpb_mlp.0.weight'].shape[0])
    hidden = int(state_dict[b0 + 'mlp.fc1.weight'].shape[0])
    ws, coords = 8, None                     # (no buffer to read the window from: the published models' 8)
    tables = [k for k in state_dict if k.endswith('attn.relative_coords_table')]
    indices = [k for k in state_dict if k.endswith('attn.relative_position_index')]
    if tables:
        shp = tuple(state_dict[tables[0]].shape)
        if len(shp) != 4 or shp[0] != 1 or shp[1] != shp[2] or shp[3] != 2 or shp[1] % 2 == 0:
            raise NotImplementedError(f'Swin2SR checkpoint: {tables[0]} has shape {shp}, not [1, 2 ws - 1, 2 ws - 1, 2]')
        ws = (shp[1] + 1) // 2
    elif indices:
        shp = tuple(state_dict[indices[0]].shape)
        ws = math.isqrt(int(shp[0])) if len(shp) == 2 else 0
        if len(shp) != 2 or shp[0] != shp[1] or ws * ws != shp[0]:
            raise NotImplementedError(f'Swin2SR checkpoint: {indices[0]} has shape {shp}, not [ws^2, ws^2]')
    if ws != 8:
        raise NotImplementedError(f'Swin2SR checkpoint with window_size {ws}: only 8 x 8 windows are built on the HIP path')
    if tables:
        coords = state_dict[tables[0]].detach().cpu().double().numpy()
        for k in tables:
            v = state_dict[k]
            if tuple(v.shape) != (1, 15, 15, 2):
                raise NotImplementedError(f'Swin2SR checkpoint: {k} has shape {tuple(v.shape)}, not (1, 15, 15, 2)')
            if not np.array_equal(v.detach().cpu().double().numpy(), coords):
                raise NotImplementedError(f'Swin2SR checkpoint: {k} differs from {tables[0]} (one relative_coords_table for every block is built on the HIP path)')
    if 'conv_up1.weight' in state_dict:
        upsampler, up = 'nearest+conv', 4 if 'conv_up2.weight' in state_dict else 2
        out_nc = int(state_dict['conv_last.weight'].shape[0])
    elif 'conv_before_upsample.0.weight' in state_dict:
        upsampler, up = 'pixelshuffle', 1
        for k, v in state_dict.items():
            if k.startswith('upsample.') and k.endswith('.weight'):
                f = math.isqrt(int(v.shape[0]) // 64)
                if f * f * 64 != int(v.shape[0]):
                    raise Exception("Could not infer model parameters.")
                up *= f
        out_nc = int(state_dict['conv_last.weight'].shape[0])
    elif 'upsample.0.weight' in state_dict:
        upsampler = 'pixelshuffledirect'
        k_up = int(state_dict['upsample.0.weight'].shape[0])
        up = math.isqrt(k_up // in_nc) if k_up % in_nc == 0 else 0
        if up * up * in_nc != k_up:
            raise NotImplementedError(f'Swin2SR checkpoint: upsample.0 has {k_up} channels, not in_chans ({in_nc}) times a square (more output than input channels is not built on the HIP path)')
        out_nc = in_nc
    else:
        raise NotImplementedError("Swin2SR checkpoint without an upsampler (upsampler '': the JPEG / denoising models): only the super-resolution forms are built on the HIP path")
    if out_nc != in_nc:
        raise NotImplementedError(f'Swin2SR checkpoint: conv_last has {out_nc} channels, conv_first takes {in_nc} (unequal channel counts are not built on the HIP path)')
    from .architectures.SwinIR_arch import relative_position_index
    want = relative_position_index(ws)
    for k in indices:
        v = state_dict[k]
        if tuple(v.shape) != tuple(want.shape) or not bool((v.cpu().long() == want).all()):
            raise NotImplementedError(f'Swin2SR checkpoint: {k} differs from (ri - rj + 7) * 15 + (ci - cj + 7), the index the engine builds its bias table with')
    state_dict = {k: v for k, v in state_dict.items() if not (k.endswith('attn.relative_position_index') or k.endswith('attn.relative_coords_table') or k.endswith('.attn_mask'))}
    cfg = {'type': 'swin2sr', 'in_nc': in_nc, 'nf': C, 'depths': depths, 'num_heads': [nh] * len(depths), 'window_size': ws, 'mlp_ratio': hidden / C, 'scale': up,
           'upsampler': upsampler, 'resi_connection': '3conv' if 'layers.0.conv.0.weight' in state_dict else '1conv', 'cpb_hidden': cpb, 'coords_table': coords}
    return dict(arch='swin2sr', scale=up, in_nc=in_nc, out_nc=in_nc, nf=C, nb=sum(depths), plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


_HAT_KEYS = ('layers.0.residual_group.blocks.0.conv_block.cab.0.weight', 'layers.0.residual_group.blocks.0.conv_block.cab.2.weight',
             'layers.0.residual_group.blocks.0.conv_block.cab.3.attention.1.weight', 'layers.0.residual_group.blocks.0.conv_block.cab.3.attention.3.weight',
             'layers.0.residual_group.overlap_attn.qkv.weight', 'layers.0.residual_group.overlap_attn.norm1.weight',
             'layers.0.residual_group.overlap_attn.relative_position_bias_table', 'layers.0.residual_group.blocks.0.attn.relative_position_bias_table')


def _infer_hat(state_dict):
    """HAT checkpoints (HAT-S, HAT, HAT-L, Real_HAT_GAN_SRx4 and fine-tunes), or None when the complete HAT key set (_HAT_KEYS) is not there -- the caller then sniffs as
    before.  embed_dim and in_chans from conv_first, depths by counting blocks, num_heads and the window from the self-attention's bias table, the overlapping window from
    the OCAB's (side = ws + ows - 1), compress_ratio / squeeze_factor from the conv block's shapes, mlp_ratio from mlp.fc1, the scale from upsample.*.  conv_scale is not in
    a state dict: 0.01, as in every published model (net_params takes another).  The two index buffers (relative_position_index_SA / _OCA) are taken out of the state dict
    handed back and passed on as rpi_sa / rpi_oca: when present they are what the dense bias tables are built from.  DRCT, an absolute position embedding, a window other
    than 16 / 24, a checkpoint without patch_embed.norm or qkv biases and unbuilt sizes are refused."""
    import math
    if any(k not in state_dict for k in _HAT_KEYS):
        return None
    b0, o0 = 'layers.0.residual_group.blocks.0.', 'layers.0.residual_group.overlap_attn.'
    if any(k.endswith('attn.logit_scale') for k in state_dict):
        raise NotImplementedError('HAT-like checkpoint with attn.logit_scale (cosine attention): not built on the HIP path')
    if any('.swin_DRCT' in k or '.adjust' in k or '.swin1.' in k for k in state_dict):
        raise NotImplementedError('HAT checkpoint with DRCT keys (.swin_DRCT / .adjust / .swin1.): neither a HAT nor a complete DRCT key set')
    if 'absolute_pos_embed' in state_dict:
        raise NotImplementedError('HAT checkpoint with absolute_pos_embed (ape=True): not built on the HIP path')
    if 'patch_embed.norm.weight' not in state_dict:
        raise NotImplementedError('HAT checkpoint without patch_embed.norm (patch_norm=False): not built on the HIP path')
    if b0 + 'attn.qkv.bias' not in state_dict or o0 + 'qkv.bias' not in state_dict:
        raise NotImplementedError('HAT checkpoint without qkv biases (qkv_bias=False): not built on the HIP path')
    for k in ('conv_first.weight', b0 + 'attn.qkv.weight', b0 + 'mlp.fc1.weight', 'conv_before_upsample.0.weight', 'conv_last.weight'):
        if k not in state_dict:
            if k.startswith('conv_before') or k == 'conv_last.weight':
                raise NotImplementedError('HAT checkpoint without the pixelshuffle tail (conv_before_upsample / conv_last): not built on the HIP path')
            raise Exception("Could not infer model parameters.")
    w0 = state_dict['conv_first.weight']
    C, in_nc = int(w0.shape[0]), int(w0.shape[1])
    depths = []
    while f'layers.{len(depths)}.residual_group.blocks.0.norm1.weight' in state_dict:
        i, j = len(depths), 0
        while f'layers.{i}.residual_group.blocks.{j}.norm1.weight' in state_dict:
            j += 1
        depths.append(j)
    table, otable = state_dict[b0 + 'attn.relative_position_bias_table'], state_dict[o0 + 'relative_position_bias_table']
    nh, side, oside = int(table.shape[1]), math.isqrt(int(table.shape[0])), math.isqrt(int(otable.shape[0]))
    ws = (side + 1) // 2
    ows = oside + 1 - ws
    if side * side != int(table.shape[0]) or 2 * ws - 1 != side or oside * oside != int(otable.shape[0]) or not depths:
        raise Exception("Could not infer model parameters.")
    if ws != 16 or ows != 24:
        raise NotImplementedError(f'HAT checkpoint with window_size {ws} and an overlapping window of {ows}: only 16 / 24 are built on the HIP path')
    if 'layers.0.conv.0.weight' in state_dict or 'layers.0.conv.weight' not in state_dict:
        raise NotImplementedError("HAT checkpoint with a resi_connection other than '1conv': not built on the HIP path")
    cc, sq = int(state_dict[_HAT_KEYS[0]].shape[0]), int(state_dict[_HAT_KEYS[2]].shape[0])
    hidden = int(state_dict[b0 + 'mlp.fc1.weight'].shape[0])
    if not (1 <= cc <= 64 and 1 <= sq <= 64):
        raise NotImplementedError(f'HAT checkpoint: a conv block of {cc} channels and a channel attention of {sq} (built on the HIP path: 1 .. 64 each)')
    up = 1
    for k, v in state_dict.items():
        if k.startswith('upsample.') and k.endswith('.weight'):
            f = math.isqrt(int(v.shape[0]) // 64)
            if f * f * 64 != int(v.shape[0]):
                raise Exception("Could not infer model parameters.")
            up *= f
    out_nc = int(state_dict['conv_last.weight'].shape[0])
    if out_nc != in_nc:
        raise NotImplementedError(f'HAT checkpoint: conv_last has {out_nc} channels, conv_first takes {in_nc} (unequal channel counts are not built on the HIP path)')
    rpi = {}
    for name, shape in (('relative_position_index_SA', (ws * ws, ws * ws)), ('relative_position_index_OCA', (ws * ws, ows * ows))):
        if name in state_dict:
            v = state_dict[name]
            if tuple(v.shape) != shape:
                raise NotImplementedError(f'HAT checkpoint: {name} has shape {tuple(v.shape)}, not {shape}')
            rpi[name] = v.cpu().long().numpy()
    state_dict = {k: v for k, v in state_dict.items() if k not in rpi and not k.endswith('.attn_mask')}
    # compress_ratio / squeeze_factor: C / n where it divides, else the smallest ratio that gives the stored channel count (C // ratio)
    ratio = lambda n: C // n if C % n == 0 else next(r for r in range(1, C + 1) if C // r == n)
    cfg = {'type': 'hat', 'in_nc': in_nc, 'nf': C, 'depths': depths, 'num_heads': [nh] * len(depths), 'window_size': ws, 'compress_ratio': ratio(cc), 'squeeze_factor': ratio(sq),
           'conv_scale': 0.01, 'overlap_ratio': (ows - ws) / ws, 'mlp_ratio': hidden / C, 'scale': up, 'upsampler': 'pixelshuffle', 'resi_connection': '1conv',
           'rpi_sa': rpi.get('relative_position_index_SA'), 'rpi_oca': rpi.get('relative_position_index_OCA')}
    return dict(arch='hat', scale=up, in_nc=in_nc, out_nc=in_nc, nf=C, nb=sum(depths), plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


# block 0's complete key set of a DAT (a window block): with before_RG.1.weight, what recognises one
_DAT_B0 = 'layers.0.blocks.0.'
_DAT_KEYS = ('conv_first.weight', 'norm.weight') + tuple(_DAT_B0 + k for k in (
    'norm1.weight', 'norm2.weight', 'attn.qkv.weight', 'attn.proj.weight', 'attn.dwconv.0.weight', 'attn.dwconv.1.running_var', 'attn.channel_interaction.1.weight',
    'attn.channel_interaction.2.running_var', 'attn.channel_interaction.4.weight', 'attn.spatial_interaction.0.weight', 'attn.spatial_interaction.1.running_var',
    'attn.spatial_interaction.3.weight', 'attn.attns.0.pos.pos_proj.weight', 'attn.attns.0.pos.pos1.0.weight', 'attn.attns.0.pos.pos1.2.weight',
    'attn.attns.0.pos.pos2.0.weight', 'attn.attns.0.pos.pos2.2.weight', 'attn.attns.0.pos.pos3.0.weight', 'attn.attns.0.pos.pos3.2.weight',
    'attn.attns.1.pos.pos_proj.weight', 'attn.attns.1.pos.pos3.2.weight', 'ffn.fc1.weight', 'ffn.sg.norm.weight', 'ffn.sg.conv.weight', 'ffn.fc2.weight'))


def _infer_dat(state_dict):
    """DAT checkpoints (DAT, DAT-S, DAT-2, DAT-light and fine-tunes).  embed_dim and in_chans from conv_first, depths by counting blocks, num_heads = 2 x the rows of
    attns.0.pos.pos3.2 (cross-checked against temperature when there is an odd block), the width of the position MLP from pos_proj, expansion_factor from ffn.fc1, '3conv',
    the tail and the scale as _infer_swinir reads them.  split_size from attns.0.rpe_biases (its last row + 1); without the buffer [8, 32] is ASSUMED and net_params says
    so (split_assumed).  If any block stores attn.attn_mask_0, the blocks that store it are the shifted ones (shift_blocks), else the published rule.  A stored rpe_biases
    feeds the position MLP; a stored relative_position_index that differs from the formula is refused; attn_mask_* values are never read.  Every buffer is dropped from
    the state dict handed back."""
    import math
    from .architectures.DAT_arch import SPLITS, relative_position_index
    b0 = _DAT_B0
    if b0 + 'attn.qkv.bias' not in state_dict:
        raise NotImplementedError('DAT checkpoint without qkv biases (qkv_bias=False): not built on the HIP path')
    w0 = state_dict['conv_first.weight']
    C, in_nc = int(w0.shape[0]), int(w0.shape[1])
    depths = []
    while f'layers.{len(depths)}.blocks.0.norm1.weight' in state_dict:
        i, j = len(depths), 0
        while f'layers.{i}.blocks.{j}.norm1.weight' in state_dict:
            j += 1
        depths.append(j)
    nh = 2 * int(state_dict[b0 + 'attn.attns.0.pos.pos3.2.weight'].shape[0])
    temp = state_dict.get('layers.0.blocks.1.attn.temperature')
    if temp is not None and int(temp.shape[0]) != nh:
        raise Exception("Could not infer model parameters.")
    pos_dim = int(state_dict[b0 + 'attn.attns.0.pos.pos_proj.weight'].shape[0])
    hidden = int(state_dict[b0 + 'ffn.fc1.weight'].shape[0])
    if not depths or C % max(nh, 1) or hidden % 2:
        raise Exception("Could not infer model parameters.")
    rpe, split_assumed = [None, None], False
    for br in (0, 1):
        v = state_dict.get(b0 + f'attn.attns.{br}.rpe_biases')
        if v is not None:
            if v.dim() != 2 or int(v.shape[1]) != 2:
                raise NotImplementedError(f'DAT checkpoint: attns.{br}.rpe_biases has shape {tuple(v.shape)}, not [rows, 2]')
            rpe[br] = v.detach().cpu().double().numpy()
    if rpe[0] is not None:
        split = (int(round(float(rpe[0][-1][0]))) + 1, int(round(float(rpe[0][-1][1]))) + 1)
    else:
        split, split_assumed = (8, 32), True
    if split not in SPLITS:
        raise NotImplementedError(f'DAT checkpoint with split_size {list(split)}: only [8, 32] and [8, 16] are built on the HIP path')
    for br, (wh, ww) in enumerate(((split[0], split[1]), (split[1], split[0]))):
        if rpe[br] is not None and rpe[br].shape != ((2 * wh - 1) * (2 * ww - 1), 2):
            raise NotImplementedError(f'DAT checkpoint: attns.{br}.rpe_biases has shape {rpe[br].shape} for a {wh} x {ww} window')
        idx = relative_position_index(wh, ww)
        for k, v in state_dict.items():
            if k.endswith(f'attn.attns.{br}.relative_position_index') and (tuple(v.shape) != tuple(idx.shape) or not bool((v.cpu().long() == idx).all())):
                raise NotImplementedError(f'DAT checkpoint: {k} differs from the published formula for a {wh} x {ww} window')
    masks = sorted((int(k.split('.')[1]), int(k.split('.')[3])) for k in state_dict if k.startswith('layers.') and k.endswith('.attn.attn_mask_0'))
    conv3 = 'layers.0.conv.0.weight' in state_dict
    if not conv3 and 'layers.0.conv.weight' not in state_dict:
        raise Exception("Could not infer model parameters.")
    if 'conv_last.weight' in state_dict and 'conv_before_upsample.0.weight' in state_dict:
        upsampler, up = 'pixelshuffle', 1
        for k, v in state_dict.items():
            if k.startswith('upsample.') and k.endswith('.weight'):
                f = math.isqrt(int(v.shape[0]) // 64)
                if f * f * 64 != int(v.shape[0]):
                    raise Exception("Could not infer model parameters.")
                up *= f
        out_nc = int(state_dict['conv_last.weight'].shape[0])
    elif 'upsample.0.weight' in state_dict:
        upsampler = 'pixelshuffledirect'
        n = int(state_dict['upsample.0.weight'].shape[0])
        up = math.isqrt(n // in_nc)
        if up * up * in_nc != n:
            raise Exception("Could not infer model parameters.")
        out_nc = in_nc
    else:
        raise NotImplementedError('DAT checkpoint without a pixelshuffle / pixelshuffledirect tail: not built on the HIP path')
    if out_nc != in_nc:
        raise NotImplementedError(f'DAT checkpoint: conv_last has {out_nc} channels, conv_first takes {in_nc} (unequal channel counts are not built on the HIP path)')
    buffers = ('.rpe_biases', '.relative_position_index', '.attn_mask_0', '.attn_mask_1')
    state_dict = {k: v for k, v in state_dict.items() if not k.endswith(buffers)}
    cfg = {'type': 'dat', 'in_nc': in_nc, 'nf': C, 'depths': depths, 'num_heads': [nh] * len(depths), 'split_size': list(split), 'expansion_factor': hidden / C, 'scale': up,
           'upsampler': upsampler, 'resi_connection': '3conv' if conv3 else '1conv', 'pos_dim': pos_dim, 'shift_blocks': masks if masks else None,
           'rpe_biases': rpe if rpe[0] is not None or rpe[1] is not None else None, 'split_assumed': split_assumed}
    return dict(arch='dat', scale=up, in_nc=in_nc, out_nc=in_nc, nf=C, nb=sum(depths), plus=False, state_dict=state_dict,
                net_params=get_network_G_config(cfg, up))


# dense group 0's complete key set of a DRCT: with conv_first.weight, what recognises one (anything less is sniffed as before)
_DRCT_KEYS = ('conv_first.weight', 'patch_embed.norm.weight', 'norm.weight', 'conv_after_body.weight') + tuple(
    f'layers.0.swin{k}.{n}' for k in range(1, 6) for n in ('norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias', 'attn.relative_position_bias_table', 'attn.qkv.weight',
                                                          'attn.qkv.bias', 'attn.proj.weight', 'attn.proj.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight',
                                                          'mlp.fc2.bias')) + tuple(f'layers.0.adjust{k}.{n}' for k in range(1, 6) for n in ('weight', 'bias'))


def _infer_drct(state_dict):
    """DRCT checkpoints (DRCT, DRCT-L, Real-DRCT-GAN and fine-tunes).  Everything is read off the shapes, which are authoritative over the published formulas: embed_dim and
    in_chans from conv_first, the dense groups by counting layers.<i>.swin1, per block the heads from relative_position_bias_table.shape[1] and the MLP's hidden size from
    mlp.fc1.weight.shape[0] (the published head rule is only cross-checked and recorded: heads_follow_rule in the dict handed back, and on the shell), gc from adjust1, the window from the table's rows, the scale
    from upsample.*.  The buffers (attn.relative_position_index, attn_mask) are dropped from the state dict handed back and never trusted for values: the engine builds the
    index from its formula -- a stored one that differs is refused -- and computes the mask from the coordinates.  What the HIP path does not build is refused here, before
    anything touches the GPU."""
    import math
    from .architectures.keys import DRCT_GC, drct_head_rule
    from .architectures.SwinIR_arch import relative_position_index
    w0 = state_dict['conv_first.weight']
    C, in_nc = int(w0.shape[0]), int(w0.shape[1])
    if 'absolute_pos_embed' in state_dict:
        raise NotImplementedError('DRCT checkpoint with absolute_pos_embed (ape=True): not built on the HIP path')
    R = 0
    while f'layers.{R}.swin1.norm1.weight' in state_dict:
        R += 1
    gc = int(state_dict['layers.0.adjust1.weight'].shape[0])
    if gc != DRCT_GC:
        raise NotImplementedError(f'DRCT checkpoint with gc {gc}: only gc 32 is built on the HIP path')
    if not 1 <= C <= 256:
        raise NotImplementedError(f'DRCT checkpoint with embed_dim {C}: up to 256 channels are built on the HIP path')
    heads, hidden = [], []
    for i in range(R):
        for k in range(5):
            b, dim = f'layers.{i}.swin{k + 1}.', C + gc * k
            for n in ('attn.relative_position_bias_table', 'attn.qkv.weight', 'mlp.fc1.weight', 'norm1.weight'):
                if b + n not in state_dict:
                    raise Exception("Could not infer model parameters.")
            table = state_dict[b + 'attn.relative_position_bias_table']
            if int(table.shape[0]) != 961:
                side = math.isqrt(int(table.shape[0]))
                raise NotImplementedError(f'DRCT checkpoint with window_size {(side + 1) // 2} ({b}attn.relative_position_bias_table has {int(table.shape[0])} rows): '
                                          'only 16 x 16 windows (961 rows) are built on the HIP path')
            if int(state_dict[b + 'norm1.weight'].shape[0]) != dim or tuple(state_dict[b + 'attn.qkv.weight'].shape) != (3 * dim, dim):
                raise NotImplementedError(f'DRCT checkpoint: {b[:-1]} does not work on C + {gc} k = {dim} channels (norm1 {tuple(state_dict[b + "norm1.weight"].shape)}, '
                                          f'qkv {tuple(state_dict[b + "attn.qkv.weight"].shape)})')
            nh, hid = int(table.shape[1]), int(state_dict[b + 'mlp.fc1.weight'].shape[0])
            if nh < 1 or nh > 8 or dim % nh or dim // nh > 128:
                raise NotImplementedError(f'DRCT checkpoint: {b[:-1]} has {nh} heads on {dim} channels (built on the HIP path: <= 8 heads of <= 128 channels, dim % heads == 0)')
            if not 1 <= hid <= 1024:
                raise NotImplementedError(f'DRCT checkpoint: {b[:-1]} has an MLP of {hid} hidden channels (built on the HIP path: <= 1024)')
            heads.append(nh); hidden.append(hid)
    if 'conv_before_upsample.0.weight' not in state_dict or 'conv_last.weight' not in state_dict or 'upsample.0.weight' not in state_dict:
        raise NotImplementedError('DRCT checkpoint without the pixelshuffle tail (conv_before_upsample / upsample / conv_last): not built on the HIP path')
    up = 1
    for k, v in state_dict.items():
        if k.startswith('upsample.') and k.endswith('.weight'):
            f = math.isqrt(int(v.shape[0]) // 64)
            if f * f * 64 != int(v.shape[0]) or int(v.shape[1]) != 64:
                raise Exception("Could not infer model parameters.")
            up *= f
    if up not in (2, 3, 4):
        raise NotImplementedError(f'DRCT checkpoint with a pixelshuffle tail of scale {up}: 2, 3 and 4 are built on the HIP path')
    out_nc = int(state_dict['conv_last.weight'].shape[0])
    if out_nc != in_nc or not 1 <= in_nc <= 4:
        raise NotImplementedError(f'DRCT checkpoint: conv_last has {out_nc} channels, conv_first takes {in_nc} (built on the HIP path: equal counts, 1 .. 4)')
    want = relative_position_index(16)
    for k in [k for k in state_dict if k.endswith('attn.relative_position_index')]:
        v = state_dict[k]
        if tuple(v.shape) != tuple(want.shape) or not bool((v.cpu().long() == want).all()):
            raise NotImplementedError(f'DRCT checkpoint: {k} differs from (ri - rj + 15) * 31 + (ci - cj + 15), the index the engine builds its bias table with')
    state_dict = {k: v for k, v in state_dict.items() if not (k.endswith('attn.relative_position_index') or k.endswith('.attn_mask'))}
    # the head count the published rule starts from: block 0 works on C channels and the rule gives num_heads - C % num_heads there (num_heads itself when it divides C)
    nh0 = heads[0]
    rule = [drct_head_rule(C + gc * k, nh0) for _ in range(R) for k in range(5)]
    cfg = {'type': 'drct', 'in_nc': in_nc, 'nf': C, 'depths': [6] * R, 'num_heads': [nh0] * R, 'window_size': 16, 'mlp_ratio': hidden[0] / C, 'scale': up,
           'upsampler': 'pixelshuffle', 'resi_connection': '1conv', 'gc': gc, 'block_heads': heads, 'block_hidden': hidden}
    info = dict(arch='drct', scale=up, in_nc=in_nc, out_nc=in_nc, nf=C, nb=5 * R, plus=False, state_dict=state_dict, net_params=get_network_G_config(cfg, up))
    info['heads_follow_rule'] = heads == rule
    return info


def _infer_pan(state_dict, scale, in_nc, out_nc):
    """PAN checkpoints: the reference leaves "custom params inference TBD" and builds the defaults
    with the caller's scale / in_nc / out_nc (run.py:157-163).  Same here when a scale is given;
    without one (the reference would fail in PAN.__init__) it is read off the up-block keys."""
    if not scale:
        ups = {int(k.split('.')[1]) for k in state_dict if k.startswith('upsample.')}
        scale = 2 ** sum(1 for i in ups if i % 5 == 1)
    cfg = {'type': 'pan', 'in_nc': in_nc, 'out_nc': out_nc}
    return dict(arch='pan', scale=int(scale), in_nc=in_nc, out_nc=out_nc, nf=40, nb=16, plus=False,
                state_dict=state_dict, net_params=get_network_G_config(cfg, int(scale)))


def _infer_ppon(state_dict, scale, in_nc, out_nc):
    """PPON checkpoints: like PAN the reference builds the defaults with the caller's scale / in_nc / out_nc
    (run.py:157-163); without a scale it is read off the reconstruction head (one up-conv per 2x)."""
    if not scale:
        idx = sorted(int(k.split('.')[1]) for k in state_dict if k.startswith('CRM.') and k.endswith('.weight'))
        scale = 2 ** (len(idx) - 2)                      # the last two convs are HR_conv0 / HR_conv1
    cfg = {'type': 'ppon', 'in_nc': in_nc, 'out_nc': out_nc}
    return dict(arch='ppon', scale=int(scale), in_nc=in_nc, out_nc=out_nc, nf=64, nb=24, plus=False,
                state_dict=state_dict, net_params=get_network_G_config(cfg, int(scale)))


def _check_out(out, shape):
    """run_u8's `out`: None, or a contiguous uint8 tensor of the result's shape."""
    if out is not None and (tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_contiguous()):
        raise ValueError(f'run_u8: out must be a contiguous uint8 tensor of shape {tuple(shape)}')


def _into_out(r, out):
    """r, or `out` (checked) holding it."""
    _check_out(out, r.shape)
    return r if out is None else out.copy_(r)


def _accepts_color_fix(fixed):
    """Decorator of Model.run_u8 / Model.run_u8_batch: the keyword color_fix=None on top of the function's own parameters.  The colour fix is a step
    BEHIND the plain call -- utils.color_fix(img, run_u8(img, ...)) -- so it is a layer around it: without the keyword the call goes straight through,
    with it the arguments are bound to the plain call's names and handed to the method `fixed` together with color_fix.  (The plain functions keep their
    parameter lists, which the tests of earlier features pin; introspection follows __wrapped__ and shows those.)"""
    import functools
    import inspect

    def layer(plain):
        sig = inspect.signature(plain)

        @functools.wraps(plain)
        def call(self, *args, color_fix=None, **kw):
            if color_fix is None:
                return plain(self, *args, **kw)
            bound = sig.bind(self, *args, **kw)
            named = dict(bound.arguments)
            del named['self']
            return getattr(self, fixed)(color_fix=color_fix, **named)
        return call
    return layer


TILE_MIN = 32            # the smallest -tile: below it the halo outweighs the core
TILE_PAD = 16            # the default -tile_pad (Real-ESRGAN's is 10; 16 = utils.SEAMLESS_PAD)


def check_tile(tile, tile_pad=TILE_PAD, chop=True):
    """The refusals of Model(tile=, tile_pad=) / `-tile N -tile_pad P`, made before anything touches the GPU: tile is None (the 200 / 0.5 chop), 0 (the whole
    image) or an int >= TILE_MIN; tile_pad an int >= 0; a tile needs chop=True (a preset that already runs whole images has nothing to tile)."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not is_int(tile_pad) or tile_pad < 0:
        raise ValueError(f'tile_pad must be an int >= 0, got {tile_pad!r}')
    if tile is None:
        return
    if not is_int(tile) or (tile != 0 and tile < TILE_MIN):
        raise ValueError(f'tile must be None (the 200 / 0.5 chop), 0 (the whole image) or an int >= {TILE_MIN}, got {tile!r}')
    if not chop:
        raise ValueError(f'tile={tile} with chop=False: this model already runs whole images')


class Model:
    def __init__(self, model_path, arch=None, scale=None, in_nc=3, out_nc=3, device='cuda',
                 meval=True, strict=True, chop=True, tile_batch=None, state_dict=None, tile=None, tile_pad=TILE_PAD):
        """tile: None -- the reference's chop (200 x 200 tiles at step 0.5, blended); 0 -- the whole image in one forward; N >= 32 -- stitched tiles of
        about N x N low-resolution pixels plus a halo of tile_pad pixels that is thrown away (tile_forward; Real-ESRGAN's --tile / --tile_pad)."""
        check_tile(tile, tile_pad, chop)
        self.tile, self.tile_pad = tile, tile_pad
        self.model_path = model_path
        self.arch = arch
        self.scale = scale
        self.in_nc = in_nc
        self.out_nc = out_nc
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("innfer_amd.Model needs device='cuda' (MI355X); the reference's -cpu mode "
                               "is not accelerated here and is not silently emulated")
        self.model = None
        self.eval = meval
        self.strict = strict
        self.chop = chop
        self.tile_batch = tile_batch
        self.load_model(state_dict)

    # ------------------------------------------------------------- loading
    def load_model(self, state_dict=None):
        if self.arch == 'ts':
            raise NotImplementedError('TorchScript models are opaque graphs and cannot run on the HIP engine')
        if state_dict is None:
            state_dict = torch.load(self.model_path, map_location='cpu')
        state_dict = unwrap_params(state_dict)
        if self.arch == 'infer':
            info = infer_from_state_dict(state_dict, self.scale, self.in_nc, self.out_nc)
            state_dict = info['state_dict']
            self.arch, self.scale = info['arch'], info['scale']
            self.in_nc, self.out_nc = info['in_nc'], info['out_nc']
            net_params = info['net_params']
        else:
            if 'n_averaged' in state_dict:
                state_dict = swa2normal(state_dict)
            if not self.scale:
                self.scale = 1
            net_params = get_network_G_config({'type': self.arch}, self.scale)
        net = get_network(net_params)
        net.load_state_dict(state_dict, strict=self.strict)
        for p in net.parameters():
            p.requires_grad = False
        if self.eval:
            net.eval()
        self.model = net.to(self.device)

    def infer_params(self, state_dict):
        return infer_from_state_dict(state_dict)['net_params']

    # ------------------------------------------------------------- forward
    def get_torch_ctx(self):
        """The context a forward runs under (run.py:204-209): torch.no_grad() -- the TorchScript special case of the reference does not arise (no
        'ts' architecture here)."""
        return torch.no_grad()

    def chop_forward(self, data, patch_size=200, step=1.0, tile_range=None):
        """Tile, run, blend (run.py:167-202).  tile_range=(begin,count) runs a
        sub-range of tiles and returns the raw HR tiles instead of the blend."""
        _, _, H, W = data.shape
        patch_size = min(H, W, patch_size)
        tiles = extract_patches_2d(data, (patch_size, patch_size), [step, step], batch_first=True,
                                   tile_range=tile_range).squeeze(0)
        from .parallel import run_tile_batches
        with torch.no_grad():
            hr = run_tile_batches(self.model, tiles, self.tile_batch, pick=self._pick if self.arch == 'ppon' else None, out=self._tile_buffer(tiles))
        if tile_range is not None:
            return hr
        return recompose_tensor(hr, H, W, step=step, scale=self.scale)

    def _tile_buffer(self, tiles):
        """The [n, C', s P_h, s P_w] buffer the blend or the stitch reads (tiles: [n, C, P_h, P_w], square on the chop path), allocated once so that every
        batch's result is written in place (no per-batch tensor + torch.cat): known for the engines that state their output shape; None (concatenate) otherwise."""
        m = self.model
        if self.arch == 'ppon' or not getattr(m, '_accepts_out', False):
            return None
        n, _, ph, pw = tiles.shape
        from .architectures.engine_module import EngineModule
        shape = m._out_shape(n, ph, pw, device=tiles.device) if isinstance(m, EngineModule) else m._out_shape(n, ph, pw)
        return torch.empty(tuple(shape), dtype=tiles.dtype, device=tiles.device)

    def _run_tiles(self, tiles):
        """The [n, C, P_h, P_w] tiles through the network in batches (parallel.run_tile_batches, PPON's pick), into the tile buffer where the engine states
        its output shape; returns the contiguous [n, C', s P_h, s P_w] results and the scale s they show."""
        from .parallel import run_tile_batches
        hr = run_tile_batches(self.model, tiles, self.tile_batch, pick=self._pick if self.arch == 'ppon' else None, out=self._tile_buffer(tiles)).contiguous()
        ph, pw = tiles.shape[2:]
        s = hr.shape[2] // ph
        if s < 1 or tuple(hr.shape[2:]) != (s * ph, s * pw):
            raise ValueError(f'tile_forward: tiles of {ph}x{pw} came back as {hr.shape[2]}x{hr.shape[3]}, not an integer multiple')
        return hr, s

    def tile_forward(self, data, tile=None, tile_pad=None):
        """Gather, run, stitch: the [1, C, H, W] tensor as equal tiles of about tile x tile pixels plus a halo of tile_pad pixels on every side that is not an
        image edge (lib.tile_plan), each through the network on its own (in batches), every result pixel copied from the one tile that owns it
        (innfer_extract_tiles_rect, innfer_stitch_tiles) -- nothing is blended, so with a halo no smaller than the network's receptive radius the result is the
        whole-image forward's bit for bit.  tile / tile_pad default to the model's."""
        from . import lib as L
        from .utils import utils as U
        tile = self.tile if tile is None else tile
        tile_pad = self.tile_pad if tile_pad is None else tile_pad
        check_tile(tile, tile_pad)
        if not tile:
            raise ValueError('tile_forward: needs a tile size (Model(tile=N) or tile=N)')
        if data.dim() != 4 or data.shape[0] != 1:
            raise NotImplementedError('tile_forward: one [1, C, H, W] image at a time')
        U._need_cuda(data, 'tile_forward')
        data = data.contiguous()
        _, Cc, H, W = data.shape
        ph, pw, ys, xs = L.tile_plan(H, W, tile, tile_pad)
        n = len(ys) * len(xs)
        with torch.no_grad(), torch.cuda.device(data.device):
            stream = torch.cuda.current_stream(data.device).cuda_stream
            tiles = torch.empty((n, Cc, ph, pw), dtype=data.dtype, device=data.device)
            L.check(L.lib.innfer_extract_tiles_rect(data.data_ptr(), U._dt(data), Cc, H, W, tile, tile_pad, 0, n, tiles.data_ptr(), stream))
            hr, s = self._run_tiles(tiles)
            del tiles
            out = torch.empty((1, hr.shape[1], s * H, s * W), dtype=hr.dtype, device=hr.device)
            L.check(L.lib.innfer_stitch_tiles(hr.data_ptr(), U._dt(hr), n, hr.shape[1], H, W, tile, tile_pad, s, out.data_ptr(), stream))
        return out

    def _whole(self, fwd, *args, **kwargs):
        """fwd(...) on a whole image; under tile=0 an allocator out-of-memory names the way out."""
        try:
            return fwd(*args, **kwargs)
        except torch.OutOfMemoryError as e:
            if self.tile == 0:
                raise torch.OutOfMemoryError(f'the whole image does not fit the GPU in one forward (-tile 0): run it in tiles, e.g. -tile 1024 or -tile 512 ({e})') from e
            raise

    def _pick(self, y):
        """PPON returns (content, structure, perceptual) and run.py keeps the last (run.py:191-192,220-221)."""
        return y[2] if self.arch == 'ppon' else y

    def _predict(self, x):
        return self._pick(self.model(x))

    @property
    def _whole_image(self):
        """Whether forwards take the whole image: chop=False, or tile=0."""
        return not self.chop or self.tile == 0

    def __call__(self, data):
        if self.chop and self.tile is None:
            return self.chop_forward(data, patch_size=200, step=0.5)
        if self.chop and self.tile:
            return self.tile_forward(data)
        with torch.no_grad():
            return self._whole(self._predict, data)

    def forward_tta(self, data):
        """The self-ensemble (`-tta`, "x8"): the mean of the eight dihedral orientations' results, turned back -- the definition run_u8(tta=True) is held
        to.  t_k = utils.dihedral(., k) on the last two axes; self(...) is __call__ (chop or whole image, PPON's pick); the sum is float32 in the order
        k = 0 .. 7 and the mean is rounded to data's dtype."""
        from .utils.utils import dihedral, dihedral_inv
        acc = None
        for k in range(8):
            y = dihedral_inv(self(dihedral(data, k)), k).float()
            acc = y if acc is None else acc + y
        return (acc * 0.125).to(data.dtype)

    @_accepts_color_fix('_run_u8_color_fix')
    def run_u8(self, img, normalize=False, fp16=True, out=None, fit_channels=False, seamless=None, outscale=None, outfilter='lanczos', tta=False):
        """Image in, image out: tensor2np(self(np2tensor(img, normalize)[.half()]), denormalize=normalize) (run.py:421-431) with the two
        conversions fused into the neighbouring kernels -- the tile gather / the blend on the chop path (_chop_u8: innfer_extract_tiles_u8_seamless,
        innfer_recompose_u8_seamless and their _fit forms, at pad = 0 / crop = 0 without a seamless mode), the first / last conv otherwise (EngineModule.forward_u8).  Bit-identical to the separate passes.
        img: uint8 HWC BGR(A), a numpy array (uploaded / downloaded as uint8) or a cuda tensor (stays on the GPU).
        fit_channels: gray (HW, HW1), gray + alpha (HW2) and BGRA images through a 3 -> 3 network (utils.fit_channels_plan): the colour plane
        as (g, g, g) / RGB, a non-constant alpha plane as (a, a, a); returns the input's layout at the network's scale.
        seamless: 'tile', 'mirror', 'replicate' or 'alpha_pad' -- the result of the image padded by SEAMLESS_PAD pixels that way (utils.seamless_pad_np),
        without the padding: bit for bit run_u8(seamless_pad_np(img, mode))[PAD s:-PAD s, PAD s:-PAD s].  On the chop path the tile gather reads the
        image through the border map and the blend stores the crop window only: neither the padded image nor the padded result exists.  Otherwise the image is padded on the GPU, run and cropped.
        outscale: the final size relative to the INPUT, int(H outscale) x int(W outscale) (Real-ESRGAN's --outscale) -- the device result is resampled
        (utils.resample, filter `outfilter`: lanczos, bicubic, bilinear, box) before it is downloaded: bit for bit utils.resample_np(run_u8(img), ...).
        Under seamless='tile' the taps wrap around, so the texture still tiles; alpha is filtered straight, not premultiplied.  `out` then has the final shape.
        tta: the self-ensemble -- bit for bit tensor2np(self.forward_tta(np2tensor(img, normalize)[.half()]), denormalize=normalize); with seamless the
        same of the padded image without the padding, with fit_channels utils.fit_channels_forward(self.forward_tta, img, ...), with outscale resampled
        as above.  On the chop path one gather fills the tiles of all eight orientations (innfer_extract_tiles_u8_tta), they run as one tile stream and
        one blend averages the eight results before it quantises (innfer_recompose_u8_tta); without chop, or where that tile buffer does not fit
        (_tta_fits), forward_tta runs on the device tensor between the existing conversions -- the same bits.
        Model(tile=N): self(...) above is tile_forward, and every definition holds with it inside.  Plain and seamless= images go through the uint8 gather
        and stitch (_tile_u8: innfer_extract_tiles_u8_rect, innfer_stitch_tiles_u8 -- neither the float image nor the padded image exists); fit_channels
        and tta run the tensor path with the tiled __call__ as the forward.  Model(tile=0) runs as chop=False does.
        color_fix (keyword only, added by _accepts_color_fix: a layer around this function, whose own parameters are those of the plain call):
        'lowfreq' (the reference's -cf), 'wavelet' or 'adain' -- by definition utils.color_fix(img, run_u8(img, <the same options without
        color_fix and outscale>), mode=color_fix), then the outscale resample.  img is the image as given: under seamless= the unpadded image against the
        cropped result, under fit_channels the image in its own layout (H x W as H x W x 1).  One upload, the network, the fix and the resample on the
        device, one download of the final image (_run_u8_color_fix)."""
        import numpy as np
        if outscale is not None:
            return self._run_u8_outscale(img, outscale, outfilter, normalize, fp16, out, fit_channels, seamless, tta)
        from .architectures.engine_module import EngineModule
        from .utils import utils as U
        host = isinstance(img, np.ndarray)
        mode = None
        if seamless is not None:
            mode = U.seamless_mode(seamless, *img.shape[:2])
            if self._whole_image:
                return self._run_u8_padded(img, seamless, normalize, fp16, out, fit_channels, tta)
        if fit_channels:
            dtype = img.dtype if host else (np.uint8 if img.dtype == torch.uint8 else np.float32)
            plan = U.fit_channels_plan(tuple(img.shape), dtype, getattr(self.model, 'in_nc', self.in_nc), getattr(self.model, 'out_nc', self.out_nc))
            if plan == 0:                                       # a 2-D image for a 1-channel network: run as H x W x 1, return H x W
                r = self.run_u8(img[:, :, None], normalize=normalize, fp16=fp16, out=None if out is None else out[:, :, None], seamless=seamless, tta=tta)
                return r[:, :, 0]
            if plan is not None:
                return self._run_u8_fit(img, plan, normalize, fp16, out, mode, tta)
        d, host = self._as_device_u8(img)
        if d.dim() != 3:
            raise TypeError('run_u8: expected a uint8 HWC image')
        with torch.no_grad(), torch.cuda.device(d.device):
            if self.chop and self.tile is None:
                out = self._chop_u8(d, normalize, fp16, out, mode=mode, tta=tta)
            elif not self._whole_image:                         # tile=N: the uint8 gather and stitch; tta through the tensor path with the tiled __call__ inside
                out = self._tta_tensor_u8(d, normalize, fp16, out, None, mode) if tta else self._tile_u8(d, normalize, fp16, out, mode)
            elif isinstance(self.model, EngineModule) and self.arch != 'ppon' and not tta:
                out = self._whole(self.model.forward_u8, d, normalize=normalize, fp16=fp16, out=out)
            else:
                out = self._whole(self._tensor_u8, d, normalize, fp16, None, self.forward_tta if tta else self._predict, out)
        return out.cpu().numpy() if host else out

    def _as_device_u8(self, img):
        """(the uint8 image on the device, contiguous; whether it came as a numpy array, so that the result is downloaded)."""
        import numpy as np
        host = isinstance(img, np.ndarray)
        d = torch.from_numpy(np.ascontiguousarray(img)).to(self.device) if host else img.contiguous()
        if d.dtype != torch.uint8:
            raise TypeError('run_u8: expected a uint8 HWC image')
        return d, host

    def _run_u8_outscale(self, img, outscale, outfilter, normalize, fp16, out, fit_channels, seamless, tta=False):
        """run_u8(outscale=): the plain call on the device, then utils.resample to int(H outscale) x int(W outscale) before the download.  A final size
        equal to the network's own result is the plain result: nothing is resampled."""
        from . import lib as L
        from .utils import utils as U
        oh, ow = U.resample_size(img.shape[0], img.shape[1], outscale)
        L.resample_filter(outfilter)
        d, host = self._as_device_u8(img)
        r = self.run_u8(d, normalize=normalize, fp16=fp16, fit_channels=fit_channels, seamless=seamless, tta=tta)
        _check_out(out, (oh, ow) + tuple(r.shape[2:]))
        with torch.cuda.device(r.device):
            r = U.resample(r, size=(oh, ow), filter=outfilter, wrap=seamless == 'tile', out=out)
        return r.cpu().numpy() if host else r

    def _run_u8_color_fix(self, img, color_fix, normalize=False, fp16=True, out=None, fit_channels=False, seamless=None, outscale=None, outfilter='lanczos', tta=False):
        """run_u8(color_fix=): the plain call on the device, utils.color_fix of the device image and the device result [, utils.resample] before the download."""
        from . import lib as L
        from .utils import utils as U
        mode = color_fix
        L.color_fix_mode(mode)
        final = None
        if outscale is not None:
            final = U.resample_size(img.shape[0], img.shape[1], outscale)
            L.resample_filter(outfilter)
        d, host = self._as_device_u8(img)
        r = self.run_u8(d, normalize=normalize, fp16=fp16, fit_channels=fit_channels, seamless=seamless, tta=tta)
        flat = r.dim() == 2                                     # fit_channels of an H x W image: fixed as H x W x 1
        lr, sr = (d[:, :, None] if d.dim() == 2 else d), (r[:, :, None] if flat else r)
        if final is None:
            _check_out(out, r.shape)
        else:
            _check_out(out, final + tuple(r.shape[2:]))
        with torch.cuda.device(r.device):
            r = U.color_fix(lr, sr, mode=mode, out=None if out is None or final is not None else (out[:, :, None] if flat else out))
            if flat:
                r = r[:, :, 0]
            if final is not None:
                r = U.resample(r, size=final, filter=outfilter, wrap=seamless == 'tile', out=out)
        return r.cpu().numpy() if host else r

    def _tta_fits(self, nbytes, device):
        """Whether the tile buffers of the eight orientations (nbytes: low-resolution tiles and their results) may be allocated: at most half of the free memory."""
        return nbytes <= torch.cuda.mem_get_info(device)[0] // 2

    def _tensor_u8(self, d, normalize, fp16, fit_C, fwd, out=None):
        """The uint8 device image d through fwd (self._predict or self.forward_tta) between the separate conversions: np2tensor / tensor2np, or under a
        fit_channels plan fit_C (1, 2, 4) fit_split / fit_merge with one fwd per plane (never one batch: train-mode BatchNorm depends on the batch).
        Returns the uint8 device result, in `out` where one is given."""
        from . import lib as L
        from .utils import utils as U
        dt, code = (torch.float16, L.F16) if fp16 else (torch.float32, L.F32)
        stream = torch.cuda.current_stream(d.device).cuda_stream
        if fit_C:
            colour, alpha, const = U.fit_split(d, normalize=normalize, dtype=dt)
            y = fwd(colour)
            ya = fwd(alpha) if alpha is not None else None
            r = U.fit_merge(y, ya, const, fit_C, denormalize=normalize, bits=8)
            return _into_out(r.view(U.fit_channels_out_shape(tuple(d.shape), int(self.scale or 1))), out)
        H, W, Cc = d.shape
        x = torch.empty((1, Cc, H, W), dtype=dt, device=d.device)
        L.check(L.lib.innfer_u8hwc_to_nchw(d.data_ptr(), H, W, Cc, int(bool(normalize)), x.data_ptr(), code, stream))
        y = fwd(x).contiguous()
        shape = (y.shape[2], y.shape[3], y.shape[1])
        _check_out(out, shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=d.device)
        L.check(L.lib.innfer_nchw_to_u8hwc(y.data_ptr(), U._dt(y), y.shape[2], y.shape[3], y.shape[1], int(bool(normalize)), out.data_ptr(), stream))
        return out

    def _tta_tensor_u8(self, d, normalize, fp16, out, fit_C, mode, fwd=None):
        """run_u8(tta=True) of the uint8 device image d without the fused kernels: _tensor_u8 with forward_tta (or another forward `fwd`), under a border
        code `mode` of the image padded in front and cropped behind."""
        from . import lib as L
        from .utils import utils as U
        fwd = fwd or self.forward_tta
        if mode is None:
            return self._tensor_u8(d, normalize, fp16, fit_C, fwd, out)
        src = U.seamless_pad(d, next(name for name, code in L.BORDER_MODES.items() if code == mode))
        return _into_out(U.seamless_crop(self._tensor_u8(src, normalize, fp16, fit_C, fwd), int(self.scale or 1)), out)

    def _tile_u8(self, d, normalize, fp16, out, mode=None):
        """The stitched tile path of run_u8 (tile=N) for the uint8 device image d: plan, gather, run the tiles, stitch -- innfer_extract_tiles_u8_rect and
        innfer_stitch_tiles_u8, np2tensor in the gather's load and tensor2np in the stitch's store, so the float image never exists.  mode: the border code
        of run_u8(seamless=): the lattice is the padded image's, the gather reads through the border map and the stitch stores the crop window only, so the
        padded image never exists either."""
        from . import lib as L
        from .utils import utils as U
        H, W, Cc = d.shape
        dt, code = (torch.float16, L.F16) if fp16 else (torch.float32, L.F32)
        stream = torch.cuda.current_stream(d.device).cuda_stream
        pad, border = (0, L.BORDER_MODES['replicate']) if mode is None else (U.SEAMLESS_PAD, mode)
        ph, pw, ys, xs = L.tile_plan(H + 2 * pad, W + 2 * pad, self.tile, self.tile_pad)
        n = len(ys) * len(xs)
        tiles = torch.empty((n, Cc, ph, pw), dtype=dt, device=d.device)
        L.check(L.lib.innfer_extract_tiles_u8_rect(d.data_ptr(), Cc, H, W, int(bool(normalize)), self.tile, self.tile_pad, 0, n, pad, border,
                                                   tiles.data_ptr(), code, stream))
        hr, s = self._run_tiles(tiles)
        del tiles
        shape = (H * s, W * s, hr.shape[1])
        _check_out(out, shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=d.device)
        L.check(L.lib.innfer_stitch_tiles_u8(hr.data_ptr(), U._dt(hr), n, hr.shape[1], H + 2 * pad, W + 2 * pad, self.tile, self.tile_pad, s,
                                             int(bool(normalize)), pad, out.data_ptr(), stream))
        return out

    def _chop_u8(self, d, normalize, fp16, out, fit_C=None, mode=None, tta=False):
        """The chop path of run_u8 for the uint8 device image d: plan, gather, run the tiles, blend -- one gather and one blend call for all four forms.
        fit_C: the fit_channels plan (1, 2, 4) or None; mode: the border code of run_u8(seamless=) or None, which is the same two kernels at pad = 0 /
        crop = 0.  tta: the tiles of all eight orientations in one buffer (8 n, with alpha 16 n), one tile stream, one blend (innfer_extract_tiles_u8_tta,
        innfer_recompose_u8_tta); where the buffers do not fit (_tta_fits, or the allocator says so) _tta_tensor_u8 returns the same bits."""
        from . import lib as L
        from .parallel import run_tile_batches
        from .utils import utils as U
        H, W = d.shape[:2]
        s = int(self.scale or 1)
        dt, code = (torch.float16, L.F16) if fp16 else (torch.float32, L.F32)
        stream = torch.cuda.current_stream(d.device).cuda_stream
        pad, border = (0, L.BORDER_MODES['replicate']) if mode is None else (U.SEAMLESS_PAD, mode)      # the lattice is the padded image's
        const = U.alpha_constant(d, fit_C) if fit_C in (2, 4) else None
        if mode == L.BORDER_MODES['alpha_pad'] and const:                   # the padding's alpha is 0: only an all-0 plane stays constant
            const = None
        alpha = fit_C in (2, 4) and const is None
        ps = min(H + 2 * pad, W + 2 * pad, 200)
        _, ys, xs = L.chop_plan(H + 2 * pad, W + 2 * pad, ps, 0.5)
        n = len(ys) * len(xs)
        count, Cin, Ct = (8 if tta else 1) * (2 if alpha else 1) * n, fit_C or d.shape[2], 3 if fit_C else d.shape[2]
        if tta and not self._tta_fits(count * Ct * ps * ps * (1 + s * s) * (2 if fp16 else 4), d.device):
            return self._tta_tensor_u8(d, normalize, fp16, out, fit_C, mode)
        try:
            tiles = torch.empty((count, Ct, ps, ps), dtype=dt, device=d.device)
            buf = self._tile_buffer(tiles)
        except torch.OutOfMemoryError:
            if not tta:
                raise
            tiles = None
            return self._tta_tensor_u8(d, normalize, fp16, out, fit_C, mode)
        if tta:
            L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), Cin, H, W, int(bool(normalize)), ps, 0.5, int(bool(fit_C)), int(alpha), pad, border,
                                                      tiles.data_ptr(), code, stream))
        else:
            gather = (d.data_ptr(), Cin, H, W, int(bool(normalize)), ps, 0.5, 0, n) + ((int(alpha),) if fit_C else ())
            L.check((L.lib.innfer_extract_tiles_u8_fit_seamless if fit_C else L.lib.innfer_extract_tiles_u8_seamless)(*gather, pad, border, tiles.data_ptr(), code, stream))
        hr = run_tile_batches(self.model, tiles, self.tile_batch, pick=self._pick if self.arch == 'ppon' else None, out=buf)
        del tiles
        if fit_C and hr.shape[1] != 3:
            raise ValueError(f'run_u8: fit_channels needs a 3-channel result, the network returned {hr.shape[1]}')
        hr = hr.contiguous()
        Co, P = hr.shape[1], hr.shape[2]
        shape = U.fit_channels_out_shape(tuple(d.shape), s) if fit_C else (H * s, W * s, Co)
        _check_out(out, shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=d.device)
        aconst = -1 if const is None else const
        if tta:
            L.check(L.lib.innfer_recompose_u8_tta(hr.data_ptr(), U._dt(hr), n, fit_C or Co, P, H + 2 * pad, W + 2 * pad, 0.5, s, U._dt(hr), int(bool(normalize)),
                                                  int(bool(fit_C)), int(alpha), aconst, pad, out.data_ptr(), stream))
        else:
            blend = (hr.data_ptr(), U._dt(hr), n) + (() if fit_C else (Co,)) + (P, H + 2 * pad, W + 2 * pad, 0.5, s, U._dt(hr), int(bool(normalize)))
            blend += (fit_C, int(alpha), aconst) if fit_C else ()
            L.check((L.lib.innfer_recompose_u8_fit_seamless if fit_C else L.lib.innfer_recompose_u8_seamless)(*blend, pad, out.data_ptr(), stream))
        return out

    # ------------------------------------------------------------- many images as one tile stream
    @_accepts_color_fix('_run_u8_batch')
    def run_u8_batch(self, imgs, normalize=False, fp16=True, seamless=None, outscale=None, outfilter='lanczos', fit_channels=False, tta=False):
        """[run_u8(img, same options) for img in imgs], bit for bit -- that is the definition.  imgs: uint8 HWC images of any sizes, all numpy arrays
        (numpy results) or all cuda tensors (cuda results).  The results of a group are views of ONE buffer -- page-locked host memory for numpy results, which
        stays locked while any of them is alive: copy what is kept for long.
        The fast path -- the 200 / 0.5 chop (chop=True, tile=None) of an eval-mode model, without fit_channels and tta -- runs the tiles of many images as
        ONE tile stream: a chop tile is ps x ps whatever its image's size, so the images are grouped by (channels, ps), result order kept; per group the
        images are packed into one buffer (numpy: one pinned staging buffer, one upload; cuda: packed on the device), ONE gather cuts all their tiles
        (innfer_extract_tiles_u8_multi), run_tile_batches runs the stream exactly as _chop_u8 runs one image's, ONE blend writes every result into one
        packed buffer (innfer_recompose_u8_multi), color_fix= fixes each result against its image in the packed upload, outscale= resamples each result on the device, and one copy into pinned memory brings a group's results
        back.  Small images then share a network launch instead of running one launch each on a fraction of the chip.  A group whose tile buffers
        (low-resolution tiles and results) exceed half of the free memory (_batch_fits: the _tta_fits rule) runs as consecutive sub-groups, and an
        allocator out-of-memory on the buffers halves the group: the same bits.  An image that is left alone in its group goes through run_u8 itself.
        Everything else -- Model(tile=N), Model(tile=0), chop=False, fit_channels, tta, a train-mode model (meval=False: BatchNorm depends on the batch) --
        loops run_u8 over the images: correct by definition, not faster.
        color_fix (keyword only, added by _accepts_color_fix as for run_u8): run_u8's; the fast path fixes every packed device result against its image
        in the packed upload before the resample."""
        return self._run_u8_batch(imgs, normalize, fp16, seamless, outscale, outfilter, fit_channels, tta)

    def _run_u8_batch(self, imgs, normalize=False, fp16=True, seamless=None, outscale=None, outfilter='lanczos', fit_channels=False, tta=False, color_fix=None):
        """run_u8_batch [with color_fix=]."""
        import numpy as np
        from .utils import utils as U
        imgs = list(imgs)
        host = [isinstance(im, np.ndarray) for im in imgs]
        if imgs and any(host) != all(host):
            raise TypeError('run_u8_batch: the images must be all numpy arrays or all cuda tensors')
        opts = dict(normalize=normalize, fp16=fp16, seamless=seamless, outscale=outscale, outfilter=outfilter, fit_channels=fit_channels, tta=tta, color_fix=color_fix)

        def plain(im):                                          # what the gather and the blend are built for; anything else is run_u8's to run or refuse
            if isinstance(im, np.ndarray):
                return im.ndim == 3 and 1 <= im.shape[2] <= 4 and im.dtype == np.uint8
            return torch.is_tensor(im) and im.is_cuda and im.dim() == 3 and 1 <= im.shape[2] <= 4 and im.dtype == torch.uint8
        if not (self.chop and self.tile is None and self.eval and not fit_channels and not tta and all(plain(im) for im in imgs)):
            return [self.run_u8(im, **opts) for im in imgs]
        if color_fix is not None:
            from . import lib as L
            L.color_fix_mode(color_fix)
        mode = None
        for im in imgs:                                         # run_u8's refusals, before anything runs
            if seamless is not None:
                mode = U.seamless_mode(seamless, im.shape[0], im.shape[1])
            if outscale is not None:
                U.resample_size(im.shape[0], im.shape[1], outscale)
        if outscale is not None:
            from . import lib as L
            L.resample_filter(outfilter)
        pad = 0 if mode is None else U.SEAMLESS_PAD
        groups = {}                                             # (C, ps) -> indices, in result order
        for i, im in enumerate(imgs):
            groups.setdefault((im.shape[2], min(im.shape[0] + 2 * pad, im.shape[1] + 2 * pad, 200)), []).append(i)
        results, waits = [None] * len(imgs), []
        with torch.no_grad():
            for idx in groups.values():
                self._chop_u8_group(imgs, idx, all(host), opts, mode, results, waits)
            for device, pinned, where in waits:                 # one synchronise for all downloads, then the split: views, no second copy
                torch.cuda.current_stream(device).synchronize()
                flat = pinned.numpy()
                for i, off, shape in where:
                    results[i] = flat[off:off + int(np.prod(shape))].reshape(shape)
        return results

    def _batch_fits(self, n_images, nbytes, device):
        """Whether n_images may run as one tile stream whose tile buffers (low-resolution tiles and their results) take nbytes: the _tta_fits rule."""
        return self._tta_fits(nbytes, device)

    def _chop_u8_group(self, imgs, idx, host, opts, mode, results, waits):
        """run_u8_batch's images imgs[i], i in idx (one channel count, one ps), as consecutive sub-groups: the longest run of images whose tile buffers fit
        (_batch_fits), halved when the allocator refuses the buffers all the same.  One image always runs, and through run_u8: alone it has nothing to share."""
        from . import lib as L
        from .utils import utils as U
        s, Cc, fp16 = int(self.scale or 1), imgs[idx[0]].shape[2], opts['fp16']
        pad = 0 if mode is None else U.SEAMLESS_PAD
        todo = list(idx)
        while todo:
            device = self.device if host else imgs[todo[0]].device
            plan = L.chop_multi_plan([imgs[i].shape[:2] for i in todo], Cc, pad, 200, 0.5, s)
            tile_bytes = Cc * plan['ps'] ** 2 * (1 + s * s) * (2 if fp16 else 4)
            n = len(todo)
            while n > 1 and not self._batch_fits(n, int(plan['first'][n]) * tile_bytes, device):
                n -= 1
            while n > 1:
                try:
                    self._chop_u8_multi(imgs, todo[:n], host, device, opts, mode, results, waits)
                    break
                except torch.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    n //= 2
            if n == 1:
                results[todo[0]] = self.run_u8(imgs[todo[0]], **opts)
            todo = todo[n:]

    def _chop_u8_multi(self, imgs, idx, host, device, opts, mode, results, waits):
        """_chop_u8 for the images imgs[i], i in idx, at once: pack, one gather, the tile stream through the network, one blend [, resample], one download.
        Device results go to results[i]; host results are read from the pinned buffer appended to `waits` once the stream has drained."""
        import numpy as np
        from . import lib as L
        from .parallel import run_tile_batches
        from .utils import utils as U
        s, Cc = int(self.scale or 1), imgs[idx[0]].shape[2]
        normalize, fp16, seamless, outscale, outfilter = (opts[k] for k in ('normalize', 'fp16', 'seamless', 'outscale', 'outfilter'))
        color_fix = opts.get('color_fix')
        dt, code = (torch.float16, L.F16) if fp16 else (torch.float32, L.F32)
        pad, border = (0, L.BORDER_MODES['replicate']) if mode is None else (U.SEAMLESS_PAD, mode)
        plan = L.chop_multi_plan([imgs[i].shape[:2] for i in idx], Cc, pad, 200, 0.5, s)
        n, ps, sizes, in_off = len(idx), plan['ps'], plan['sizes'], plan['in_off']
        total = int(plan['first'][n])

        def upload(records):                                    # a table of the plan: pinned, then one asynchronous copy
            t = torch.empty(records.nbytes, dtype=torch.uint8, pin_memory=True)
            t.numpy()[:] = records.view(np.uint8)
            return t.to(device, non_blocking=True)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            tiles = torch.empty((total, Cc, ps, ps), dtype=dt, device=device)
            buf = self._tile_buffer(tiles)
            if host:                                            # every image into one pinned staging buffer, one upload
                stage = torch.empty(int(in_off[n]), dtype=torch.uint8, pin_memory=True)
                flat = stage.numpy()
                for j, i in enumerate(idx):
                    flat[in_off[j]:in_off[j] + imgs[i].size] = imgs[i].reshape(-1)
                d = stage.to(device, non_blocking=True)
            else:                                               # packed on the device
                d = torch.empty(int(in_off[n]), dtype=torch.uint8, device=device)
                for j, i in enumerate(idx):
                    d[in_off[j]:in_off[j] + imgs[i].numel()].view(imgs[i].shape).copy_(imgs[i])
            table = upload(plan['tiles'])
            L.check(L.lib.innfer_extract_tiles_u8_multi(d.data_ptr(), n, sizes.ctypes.data, Cc, int(bool(normalize)), 200, 0.5, pad, border, table.data_ptr(),
                                                        tiles.data_ptr(), code, stream))
            hr = run_tile_batches(self.model, tiles, self.tile_batch, pick=self._pick if self.arch == 'ppon' else None, out=buf)
            del tiles, table
            if color_fix is None:
                del d
            hr = hr.contiguous()
            Co, P = hr.shape[1], hr.shape[2]
            if Co != Cc:                                        # the packed results hold the network's channel count
                plan = L.chop_multi_plan([imgs[i].shape[:2] for i in idx], Co, pad, 200, 0.5, s)
            out_off = plan['out_off']
            out = torch.empty(int(out_off[n]), dtype=torch.uint8, device=device)
            frames = upload(plan['images'])
            L.check(L.lib.innfer_recompose_u8_multi(hr.data_ptr(), U._dt(hr), n, sizes.ctypes.data, Co, P, 200, 0.5, s, U._dt(hr), int(bool(normalize)), pad,
                                                    frames.data_ptr(), out.data_ptr(), stream))
            del hr, frames
            shapes = [(int(h) * s, int(w) * s, Co) for h, w in sizes]
            res = [out[out_off[j]:out_off[j] + int(np.prod(shapes[j]))].view(shapes[j]) for j in range(n)]
            if color_fix is not None:                           # run_u8's definition: utils.color_fix of each image in the packed upload and its device result
                lrs = [d[in_off[j]:in_off[j] + int(h) * int(w) * Cc].view(int(h), int(w), Cc) for j, (h, w) in enumerate(sizes)]
                out = torch.empty_like(out)
                res = [U.color_fix(lr, r, mode=color_fix, out=out[out_off[j]:out_off[j] + int(np.prod(shapes[j]))].view(shapes[j]))
                       for j, (lr, r) in enumerate(zip(lrs, res))]
                del d, lrs
            if outscale is not None:                            # run_u8's definition: utils.resample of each device result, here into one packed buffer
                finals = [U.resample_size(int(h), int(w), outscale) + (Co,) for h, w in sizes]
                off = np.concatenate(([0], np.cumsum([-(-int(np.prod(f)) // 16) * 16 for f in finals])))
                out = torch.empty(int(off[n]), dtype=torch.uint8, device=device)
                res = [U.resample(r, size=f[:2], filter=outfilter, wrap=seamless == 'tile', out=out[off[j]:off[j] + int(np.prod(f))].view(f))
                       for j, (r, f) in enumerate(zip(res, finals))]
                shapes, out_off = finals, off
            if not host:
                for j, i in enumerate(idx):
                    results[i] = res[j]
                return
            pinned = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
            pinned.copy_(out, non_blocking=True)
            waits.append((device, pinned, [(i, int(out_off[j]), shapes[j]) for j, i in enumerate(idx)]))

    def _run_u8_padded(self, img, seamless, normalize, fp16, out, fit_channels, tta=False):
        """run_u8(seamless=) where the chop kernels do not apply (whole-image forwards): pad on the GPU (innfer_pad_inthwc), run as without the switch,
        crop on the GPU."""
        from .utils import utils as U
        d, host = self._as_device_u8(img)
        r = self.run_u8(U.seamless_pad(d, seamless), normalize=normalize, fp16=fp16, fit_channels=fit_channels, tta=tta)
        r = _into_out(U.seamless_crop(r, int(self.scale or 1)), out)
        return r.cpu().numpy() if host else r

    def _run_u8_fit(self, img, C, normalize, fp16, out, mode=None, tta=False):
        """run_u8(fit_channels=True) of an HW / HWC (C 1, 2, 4) uint8 image with a 3 -> 3 network.  Chop: the colour tiles and the alpha tiles
        (none when the alpha plane is constant) are gathered into one buffer, run as one tile stream and blended in one pass
        (_chop_u8: the FIT forms of the gather and the blend).  Otherwise the two planes are split, run as separate forwards (never one batch:
        train-mode BatchNorm depends on the batch) and merged (innfer_inthwc_to_nchw_fit / innfer_nchw_to_inthwc_fit).
        mode: the border code of run_u8(seamless=) on the chop path."""
        from .utils import utils as U
        d, host = self._as_device_u8(img)
        _check_out(out, U.fit_channels_out_shape(tuple(d.shape), int(self.scale or 1)))
        with torch.no_grad(), torch.cuda.device(d.device):
            if self.chop and self.tile is None:
                out = self._chop_u8(d, normalize, fp16, out, fit_C=C, mode=mode, tta=tta)
            elif not self._whole_image:                         # tile=N: the tensor path, one tiled __call__ per plane
                out = self._tta_tensor_u8(d, normalize, fp16, out, C, mode, self.forward_tta if tta else self)
            else:
                out = self._whole(self._tensor_u8, d, normalize, fp16, C, self.forward_tta if tta else self._predict, out)
        return out.cpu().numpy() if host else out


# ------------------------------------------------------------------- command line (run.py:225-445)
def parse_models(models_paths, scales_list=None):
    """`a+b` / `a>b` model chains and the per-model scale guessed from the file name (run.py:227-250)."""
    from .utils.utils import get_models_paths
    model_chain = models_paths.split("+") if "+" in models_paths else models_paths.split(">")
    try:
        all_models = get_models_paths("./models")
    except AssertionError:          # the reference insists on a ./models folder even for absolute paths; only the partial-name search needs it
        all_models = []
    full_chain = [check_model_path(m, all_models) for m in model_chain]
    if not scales_list:
        scales_list = [get_scale_name(m, None) for m in full_chain]
    elif len(scales_list) != len(model_chain):
        raise ValueError(f"The num. of scales {len(scales_list)} is != from number of models {len(model_chain)}")
    return full_chain, scales_list


def check_model_path(model_path, all_models=None):
    """Absolute path, ./models/<name>, or a unique partial-name match in ./models (run.py:253-274)."""
    import os.path as osp
    if osp.isfile(model_path):
        return model_path
    model_path_a = osp.join("models", model_path)
    if osp.isfile(model_path_a):
        return model_path_a
    if not all_models:
        raise ValueError(f"Model {model_path} not found.")
    m_list = [m for m in all_models if str(model_path.lower()) in str(m).lower()]
    if len(m_list) > 1:
        raise ValueError(f"Filter {model_path} returned multiple models: {m_list}.")
    if not m_list:
        raise ValueError(f"Model {model_path} not found.")
    return m_list[0]


def get_scale_name(model_path, scale=None):
    """The scale a model file announces in the first two characters of its name -- `4x_name.pth` -> 4, `x2net.pth` -> 2 -- or None; an explicit
    `scale` wins, with the reference's warning when the name disagrees (run.py:277-293)."""
    import os.path as osp
    import re
    head = osp.basename(model_path)[:2].lower()
    digits = head.replace('x', '')
    from_name = int(digits) if 'x' in head and re.fullmatch(r'[+-]?\d+', digits.strip()) else None
    if not scale:
        return from_name
    if from_name and from_name != scale:
        print(f"Warning: possible model scale mismatch on {model_path}")
    return scale


SEAMLESS_CHOICES = ('tile', 'mirror', 'replicate', 'alpha_pad')           # utils.SEAMLESS_MODES
OUTFILTER_CHOICES = ('lanczos', 'bicubic', 'bilinear', 'box')             # utils.RESAMPLE_FILTERS
CF_MODE_CHOICES = ('lowfreq', 'wavelet', 'adain')                         # utils.COLOR_FIX_MODES

pix2pix_extras = {'meval': False, 'strict': True, 'normalize': True}       # run.py:299-303
cyglegan_extras = {'meval': True, 'strict': False, 'normalize': True}      # run.py:305-309
default_extras = {'meval': True, 'strict': True, 'normalize': False}       # run.py:311-315


def build_parser():
    """The reference's flags, names and destinations (run.py:320-331)."""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('-models', '-m', type=str, required=True, help='Path to models.')
    parser.add_argument('-arch', '-a', type=str, required=False, default='infer', help='Model architecture.')
    parser.add_argument('-input', '-i', type=str, required=False, default='./input', help='Path to read input images.')
    parser.add_argument('-output', '-o', type=str, required=False, default='./output', help='Path to save output images.')
    parser.add_argument('-scale', '-s', type=str, required=False, default='-1', help='Model scaling factor.')
    parser.add_argument('-cf', required=False, action='store_true', help='Use color correction if enabled.')
    parser.add_argument('-comp', required=False, action='store_true', help='Save as comparison images if enabled.')
    parser.add_argument('-no_gpu', '-cpu', required=False, action='store_false', help='Run in CPU if enabled.')
    parser.add_argument('-no_fp16', required=False, action='store_false', help='Disable fp16 mode if needed.')
    parser.add_argument('-norm', required=False, action='store_true', help='Normalizes images in range [-1,1] if set, else [0,1].')
    # not a reference flag: absent from the parsed namespace unless given, so the reference's flags parse to exactly what they did
    parser.add_argument('-fit_channels', required=False, action='store_true', default=argparse.SUPPRESS,
                        help='Run gray, gray + alpha and RGBA images through RGB models (alpha as a gray image through the model).')
    parser.add_argument('-seamless', required=False, choices=SEAMLESS_CHOICES, default=argparse.SUPPRESS,
                        help='Upscale tileable textures without a seam: the image is padded by 16 px (tile: wrap around, mirror, replicate: edge pixels, '
                             'alpha_pad: transparent black) and the padding is cut off the result.')
    parser.add_argument('-outscale', required=False, type=float, default=argparse.SUPPRESS,
                        help='Final size relative to the input, e.g. 2 or 2.5 with a 4x model: the result is resampled on the GPU before it is downloaded.')
    parser.add_argument('-outfilter', required=False, choices=OUTFILTER_CHOICES, default=argparse.SUPPRESS,
                        help='Filter of -outscale (default lanczos); antialiased when it reduces.')
    parser.add_argument('-cf_mode', required=False, choices=CF_MODE_CHOICES, default=argparse.SUPPRESS,
                        help='The colour correction (given alone it turns the correction on; -cf alone is lowfreq).  lowfreq: the low-frequency LR - SR difference '
                             'in linear light; wavelet: the result keeps its own detail and takes the input\'s colours below about 63 px (five a-trous levels, '
                             'StableSR\'s wavelet fix); adain: every channel is moved to the input\'s mean and standard deviation.')
    parser.add_argument('-tta', required=False, action='store_true', default=argparse.SUPPRESS,
                        help='Self-ensemble ("x8"): run the image in its eight flipped / rotated orientations and average the results before quantisation; '
                             'eight times the network cost.')
    parser.add_argument('-tile', required=False, type=int, default=argparse.SUPPRESS,
                        help=f'Stitch large tiles instead of blending 200 x 200 ones: tiles of about N x N pixels (N >= {TILE_MIN}, e.g. 512 or 1024) plus a halo '
                             'that is thrown away, about 1.1x the image through the network where the default runs 3.7x or more.  0: the whole image in one forward.')
    parser.add_argument('-tile_pad', required=False, type=int, default=argparse.SUPPRESS,
                        help=f'Halo of -tile in pixels (default {TILE_PAD}): context on every tile side that is not an image edge.')
    parser.add_argument('-batch', required=False, type=int, default=argparse.SUPPRESS,
                        help='Run up to B consecutive images as one tile stream (B >= 1): the 200 x 200 tiles of images that share a channel count and a tile '
                             'size go through the network together, so folders of small images (sprites, texture tiles) fill the GPU.  The files written are '
                             'those of a run without the flag.  Measured with 64 images: 3 - 27x the images/s at 64 x 64 .. 128 x 128 (B 4 .. 64), 1.5 - 2.2x at 256 x 256, '
                             '1.1 - 1.25x from 512 x 512 on; B = 1 shares nothing and is up to 12 %% slower for very fast models on small images.  '
                             'Not with -tile or the whole-image presets.')
    return parser


def main(argv=None):
    """The image loop of the reference's command line (run.py:318-445) on the HIP engine: same flags, same per-architecture presets, same
    sequence read -> [linear_resize | modcrop] -> np2tensor -> model chain [-> guided filter] -> tensor2np [-> color_fix] -> save.  The
    uint8 image is what crosses PCIe in both directions; files go through OpenCV when it is installed and through PIL otherwise."""
    import os
    import os.path as osp
    import numpy as np
    from .utils import utils as U
    args = build_parser().parse_args(argv)
    if not args.no_gpu:
        raise RuntimeError("-cpu / -no_gpu: innfer_amd runs on an MI355X only; use the reference for a CPU run")
    if args.arch == 'ts':
        raise NotImplementedError('TorchScript models are opaque graphs and cannot run on the HIP engine')
    fp16 = args.no_fp16
    use_guided_filter = use_modcrop = False
    if 'unet_' in args.arch or 'p2p_' in args.arch:
        defaults, chop = pix2pix_extras, False
        resize = 512 if '512' in args.arch else 256 if '256' in args.arch else 128 if '128' in args.arch else False
    elif 'resnet_' in args.arch or 'cg_' in args.arch:
        defaults, chop, resize = cyglegan_extras, True, False
    elif 'wbc' in args.arch or 'wbc' in args.models:
        args.arch = "wbcunet_tf" if ('tf' in args.arch or 'tf' in args.models) else "wbcunet"
        defaults, chop, resize = pix2pix_extras, False, False
        use_guided_filter = use_modcrop = True
    else:
        defaults, resize, chop = default_extras, False, True
    seamless = getattr(args, 'seamless', None)
    if seamless and resize:
        raise ValueError(f"-seamless {seamless} with '{args.arch}': the preset enlarges every image to a multiple of {resize} px first, which no tileable "
                         "texture survives; resize the texture yourself and run it without the preset")
    tile, tile_pad = getattr(args, 'tile', None), getattr(args, 'tile_pad', TILE_PAD)
    if tile is None and hasattr(args, 'tile_pad'):
        raise ValueError('-tile_pad is the halo of -tile N: give both')
    if tile is not None and not chop:
        raise ValueError(f"-tile {tile} with '{args.arch}': the preset already runs every image whole, there is nothing to tile")
    check_tile(tile, tile_pad, chop)
    batch = getattr(args, 'batch', None)
    if batch is not None:
        if batch < 1:
            raise ValueError(f'-batch must be an int >= 1, got {batch}')
        if tile is not None:
            raise ValueError(f'-batch {batch} with -tile {tile}: only the tiles of the default 200 x 200 chop share a tile stream; drop one of the two')
        if not chop:
            raise ValueError(f"-batch {batch} with '{args.arch}': the preset runs every image whole, there are no tiles to share a launch")
    tta = getattr(args, 'tta', False)
    outscale, outfilter = getattr(args, 'outscale', None), getattr(args, 'outfilter', 'lanczos')
    cf_mode = getattr(args, 'cf_mode', 'lowfreq' if args.cf else None)      # None: no colour correction
    if outscale is not None:
        U.resample_size(1, 1, outscale)                     # ValueError unless 0 < F < inf
    meval, strict = defaults['meval'], defaults['strict']
    normalize = defaults['normalize'] or args.norm
    device = torch.device('cuda')
    scale = args.scale if args.scale != -1 else None        # (sic) the string '-1' never equals -1: the flag's value is what parse_models ignores
    del scale
    model_chain, scale_chain = parse_models(args.models)
    models = [Model(mc, args.arch, sc, device=device, meval=meval, strict=strict, chop=chop, tile=tile, tile_pad=tile_pad) for mc, sc in zip(model_chain, scale_chain)]
    if not fp16:
        # -no_fp16 = fp32 arithmetic on the GPU (run.py:345,421-422).  RRDBNet / SRResNet have an fp32-accurate engine, every other shipped generator an fp32
        # mode (float32 tensors select them).  The check stays for an engine built fp16-only: it must refuse, not hand out fp16 accuracy under the flag.
        from .architectures.engine_module import EngineModule
        for m in models:
            if not getattr(m.model, '_has_fp32', isinstance(m.model, EngineModule)):      # (an EngineModule has the fp32-accurate engine unless it says otherwise: SRVGGNetCompact)
                raise NotImplementedError(f"-no_fp16: no fp32-accurate engine is built for '{m.arch}' ({type(m.model).__name__}); drop the flag to run its fp16 engine")
    fit_channels = getattr(args, 'fit_channels', False)
    if fit_channels:
        ins = [getattr(m.model, 'in_nc', m.in_nc) for m in models]
        outs = [getattr(m.model, 'out_nc', m.out_nc) for m in models]

        def fit_plan(im):
            # utils.fit_channels_plan for the chain: 0 (H x W for a 1-channel first network) as it says; 1, 2, 4 only when every network is 3 -> 3
            plan = U.fit_channels_plan(im.shape, im.dtype, ins[0], outs[-1])
            return plan if plan == 0 or all(i == o == 3 for i, o in zip(ins, outs)) else None

    def chain(t_in):                        # the tensor path of an image or of one fit_channels plane: the chain [with the guided filter, its own input as the guide]
        t = t_in
        for mod in models:
            t = mod.forward_tta(t) if tta else mod(t)
            if use_guided_filter:
                t = U.guided_filter(t_in, t, r=1, eps=5e-3)
        return t
    images = U.get_images_paths(args.input)
    os.makedirs(args.output, exist_ok=True)
    # The loop is pipelined over the images: one thread decodes the next image file while the GPU works on this one, up to sixteen threads
    # encode and write finished images (PNG coding releases the GIL and is the slowest stage by far: profiles/r2/cli_pipeline.txt).  Everything that touches the GPU stays on this thread; outputs and messages are those
    # of the serial loop, in its order.
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor

    def save(img, img_out, path):
        if args.comp:
            U.save_img_comp([img, img_out], path)
        else:
            U.save_img(img_out, path)

    n_writers = max(2, min(16, os.cpu_count() or 2))
    reader, writer, pending = ThreadPoolExecutor(1), ThreadPoolExecutor(n_writers), deque()
    last_write = {}                 # output path -> future of the last write submitted for it

    def save_after(prev, img, img_out, path):
        # a/x.png and b/x.png (or x.png and x.jpg) share output/x.png: the reference's serial loop keeps the LAST one, so writes to one path are chained
        if prev is not None:
            prev.result()
        save(img, img_out, path)
    def before(img):
        # an image as it was read -> what the network step and the steps behind it need of it
        if resize:
            img = U.linear_resize(img, resize)
        if use_modcrop:
            img = U.modcrop(img, 4)
        plan = fit_plan(img) if fit_channels else None
        flat = plan is not None and img.ndim == 2                                   # a 2-D image runs as H x W x 1 and is saved 2-D
        if flat:
            img = img[:, :, None]
        single = len(models) == 1 and not use_guided_filter and img.dtype == np.uint8
        sm = {'seamless': seamless} if seamless else {}                             # run_u8 pads and crops inside its kernels
        if tta:
            sm['tta'] = True
        final = U.resample_size(img.shape[0], img.shape[1], outscale) if outscale is not None else None      # relative to the image fed to the chain
        in_run_u8 = single and (plan or img.ndim == 3)                              # the network step is run_u8 / run_u8_batch: the fix and the resample go into it
        if final and (in_run_u8 or not cf_mode):                                    # run_u8 resamples before the download
            sm.update(outscale=outscale, outfilter=outfilter)
        if cf_mode and in_run_u8:
            sm['color_fix'] = cf_mode
        src = img
        if seamless and not in_run_u8:                   # chains, 16-bit images, the guided filter: pad once in front, crop behind
            img = U.seamless_pad(img, seamless)
        return img, src, plan, flat, single, sm, final

    def network(img, plan, single, sm):
        if plan and single:                                                         # plan 1, 2, 4: colour (+ alpha) planes
            return models[0].run_u8(img, normalize=normalize, fp16=fp16, fit_channels=True, **sm)
        if plan:
            return U.fit_channels_forward(chain, img, normalize=normalize, device=device, dtype=torch.float16 if fp16 else torch.float32)
        if single and img.ndim == 3:
            return models[0].run_u8(img, normalize=normalize, fp16=fp16, **sm)       # conversions fused into the tile gather / blend / first and last conv
        t_img = U.np2tensor(img, normalize=normalize, device=device, dtype=torch.float16 if fp16 else torch.float32)
        return U.tensor2np(chain(t_img).detach(), denormalize=normalize)

    def after(image_path, img, src, flat, final, img_out, fixed):
        if img is not src:                                                          # padded in front of the chain: PAD x the chain's scale off every side
            total = 1
            for mod in models:
                total *= int(mod.scale or 1)
            img, img_out = src, U.seamless_crop(img_out, total)
        if cf_mode and not fixed:
            img_out = U.color_fix(img, img_out, mode=cf_mode)
        if final and img_out.shape[:2] != final:                                    # not done inside run_u8: chains, -cf, 16-bit images, the guided filter
            img_out = U.resample(img_out, size=final, filter=outfilter, wrap=seamless == 'tile')
        if flat:
            img, img_out = img[:, :, 0], img_out[:, :, 0]
        img_name = osp.splitext(osp.basename(image_path))[0]
        out_path = osp.join(args.output, f'{img_name:s}.png')
        fut = writer.submit(save_after, last_write.get(out_path), img, img_out, out_path)
        last_write[out_path] = fut
        pending.append(fut)
        while len(pending) > n_writers:           # a bounded number of finished images wait for their files (an 8K RGB output is 100 MB)
            pending.popleft().result()

    # -batch B: B consecutive images make a round -- the reader is B files ahead, the round's plain images (uint8, 3-D, one model, no guided filter, no
    # fit_channels plan) go through run_u8_batch as one tile stream and every other image through the per-image step; what follows the network is per image.
    ahead = batch or 1
    reads = deque(reader.submit(U.read_img, path) for path in images[:ahead])
    try:
        for start in range(0, len(images), ahead):
            ready = []
            for idx in range(start, min(start + ahead, len(images))):
                img = reads.popleft().result()
                if idx + ahead < len(images):
                    reads.append(reader.submit(U.read_img, images[idx + ahead]))
                if img is None:
                    print(f'Error reading image {images[idx]}, skipping.')
                    continue
                ready.append((images[idx],) + before(img))
            together = [k for k, (_, img, _, plan, _, single, _, _) in enumerate(ready) if batch and single and not plan and img.ndim == 3]
            batched = {}
            if together:
                opts = ready[together[0]][6]                                            # the same for every image of a run
                batched = dict(zip(together, models[0].run_u8_batch([ready[k][1] for k in together], normalize=normalize, fp16=fp16, **opts)))
            for k, (image_path, img, src, plan, flat, single, sm, final) in enumerate(ready):
                after(image_path, img, src, flat, final, batched.pop(k) if k in batched else network(img, plan, single, sm), 'color_fix' in sm)
        while pending:
            pending.popleft().result()
    finally:
        reader.shutdown(wait=True)
        writer.shutdown(wait=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
