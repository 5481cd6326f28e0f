"""Per-architecture default hyper-parameters: mirror of the reference's
utils/defaults.py:3-147 for the families on the HIP hot path.  Same input
contract (a kind string or a dict with 'type' / 'which_model_G'), same output keys,
so configs written for the reference resolve identically."""

SEAMLESS_PAD = 16          # low-resolution pixels the seamless modes pad on every side (utils.seamless_pad, Model.run_u8(seamless=), `run.py -seamless`)

_RRDB = ('rrdb_net', 'esrgan', 'evsrgan', 'esrgan-lite')
_SRRES = ('sr_resnet', 'srresnet', 'srgan')


def _pick(src, name, default):
    return src.pop(name, default)


def get_network_G_config(network_G, scale):
    scale = int(scale)
    if isinstance(network_G, str):
        kind, opts = network_G.lower(), {}
    elif isinstance(network_G, dict):
        opts = network_G
        name_key = 'which_model_G' if 'which_model_G' in opts else 'type'
        kind = opts.pop(name_key).lower()
    else:
        raise TypeError('network_G must be a str or a dict')

    cfg = {}
    if kind in _RRDB:
        lite = kind == 'esrgan-lite'
        cfg['type'] = 'rrdb_net'
        cfg['norm_type'] = _pick(opts, 'norm_type', None)
        cfg['mode'] = _pick(opts, 'mode', 'CNA')
        cfg['nf'] = _pick(opts, 'nf', 32 if lite else 64)
        cfg['nb'] = _pick(opts, 'nb', 12 if lite else 23)
        cfg['nr'] = _pick(opts, 'nr', 3)
        cfg['in_nc'] = _pick(opts, 'in_nc', 3)
        cfg['out_nc'] = _pick(opts, 'out_nc', 3)
        cfg['gc'] = _pick(opts, 'gc', 32)
        cfg['convtype'] = _pick(opts, 'convtype', 'Conv3D' if kind == 'evsrgan' else 'Conv2D')
        cfg['act_type'] = _pick(opts, 'net_act', None) or _pick(opts, 'act_type', 'leakyrelu')
        cfg['gaussian_noise'] = _pick(opts, 'gaussian', True)
        cfg['plus'] = _pick(opts, 'plus', False)
        cfg['finalact'] = _pick(opts, 'finalact', None)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['upsample_mode'] = _pick(opts, 'upsample_mode', 'upconv')
    elif kind in _SRRES:
        cfg['type'] = 'sr_resnet'
        cfg['in_nc'] = _pick(opts, 'in_nc', 3)
        cfg['out_nc'] = _pick(opts, 'out_nc', 3)
        cfg['nf'] = _pick(opts, 'nf', 64)
        cfg['nb'] = _pick(opts, 'nb', 16)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['norm_type'] = _pick(opts, 'norm_type', None)
        cfg['act_type'] = _pick(opts, 'net_act', None) or _pick(opts, 'act_type', 'relu')
        cfg['mode'] = _pick(opts, 'mode', 'CNA')
        cfg['upsample_mode'] = _pick(opts, 'upsample_mode', 'pixelshuffle')
        cfg['convtype'] = _pick(opts, 'convtype', 'Conv2D')
        cfg['finalact'] = _pick(opts, 'finalact', None)
        cfg['res_scale'] = _pick(opts, 'res_scale', 1)
    elif 'wbcunet' in kind:
        cfg['type'] = 'wbcunet_net'
        cfg['nf'] = _pick(opts, 'nf', 32)
        cfg['mode'] = 'tf' if 'tf' in kind else _pick(opts, 'mode', 'pt')
    elif 'unet' in kind or 'p2p' in kind:
        cfg['type'] = 'unet_net'
        cfg['input_nc'] = _pick(opts, 'in_nc', 3)
        cfg['output_nc'] = _pick(opts, 'out_nc', 3)
        cfg['num_downs'] = _pick(opts, 'num_downs', 7 if kind in ('unet_128', 'p2p_128') else 8)
        cfg['ngf'] = _pick(opts, 'ngf', 64)
        cfg['norm_type'] = _pick(opts, 'norm_type', 'batch')
        cfg['use_dropout'] = _pick(opts, 'use_dropout', False)
        cfg['upsample_mode'] = _pick(opts, 'upsample_mode', 'deconv')
    elif kind in ('pan_net', 'pan'):
        cfg['type'] = 'pan_net'
        cfg['in_nc'] = _pick(opts, 'in_nc', 3)
        cfg['out_nc'] = _pick(opts, 'out_nc', 3)
        cfg['nf'] = _pick(opts, 'nf', 40)
        cfg['unf'] = _pick(opts, 'unf', 24)
        cfg['nb'] = _pick(opts, 'nb', 16)
        cfg['scale'] = _pick(opts, 'scale', scale)
        cfg['self_attention'] = _pick(opts, 'self_attention', True)
        cfg['double_scpa'] = _pick(opts, 'double_scpa', False)
        cfg['ups_inter_mode'] = _pick(opts, 'ups_inter_mode', 'nearest')
    elif 'ppon' in kind:
        cfg['type'] = 'ppon'
        cfg['in_nc'] = _pick(opts, 'in_nc', 3)
        cfg['out_nc'] = _pick(opts, 'out_nc', 3)
        cfg['nf'] = _pick(opts, 'nf', 64)
        cfg['nb'] = _pick(opts, 'nb', 24)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['act_type'] = _pick(opts, 'net_act', None) or _pick(opts, 'act_type', 'leakyrelu')
        cfg['alpha'] = _pick(opts, 'alpha', 1)
    elif ('resnet' in kind and kind != 'sr_resnet') or 'cg' in kind:
        cfg['type'] = 'resnet_net'
        cfg['input_nc'] = _pick(opts, 'in_nc', 3)
        cfg['output_nc'] = _pick(opts, 'out_nc', 3)
        cfg['n_blocks'] = _pick(opts, 'n_blocks', 6 if kind in ('resnet_6blocks', 'resnet_6', 'cg_6') else 9)
        cfg['ngf'] = _pick(opts, 'ngf', 64)
        cfg['norm_type'] = _pick(opts, 'norm_type', 'instance')
        cfg['use_dropout'] = _pick(opts, 'use_dropout', False)
        cfg['upsample_mode'] = _pick(opts, 'upsample_mode', 'deconv')
        cfg['padding_type'] = _pick(opts, 'padding_type', 'reflect')
    elif kind in ('mrrdb_net', 'mesrgan'):                 # modified ("new"-arch) ESRGAN (defaults.py:45-52)
        cfg['type'] = 'mrrdb_net'
        cfg['in_nc'] = _pick(opts, 'in_nc', 3)
        cfg['out_nc'] = _pick(opts, 'out_nc', 3)
        cfg['nf'] = _pick(opts, 'nf', 64)
        cfg['nb'] = _pick(opts, 'nb', 24)
        cfg['gc'] = _pick(opts, 'gc', 32)
    elif kind in ('realesrgan_net', 'realesrgan'):         # BasicSR's RRDBNet (the Real-ESRGAN releases): its own constructor surface
        cfg['type'] = 'realesrgan_net'
        cfg['num_in_ch'] = _pick(opts, 'in_nc', 3)
        cfg['num_out_ch'] = _pick(opts, 'out_nc', 3)
        cfg['scale'] = _pick(opts, 'scale', scale)
        cfg['num_feat'] = _pick(opts, 'nf', 64)
        cfg['num_block'] = _pick(opts, 'nb', 23)
        cfg['num_grow_ch'] = _pick(opts, 'gc', 32)
    elif kind in ('compact_net', 'compact'):               # BasicSR's SRVGGNetCompact (realesr-animevideov3 / general-x4v3, "compact" models): its own constructor surface
        cfg['type'] = 'compact_net'
        cfg['num_in_ch'] = _pick(opts, 'in_nc', 3)
        cfg['num_out_ch'] = _pick(opts, 'out_nc', 3)
        cfg['num_feat'] = _pick(opts, 'nf', 64)
        cfg['num_conv'] = _pick(opts, 'nb', 16)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['act_type'] = _pick(opts, 'act_type', 'prelu')
    elif kind in ('span_net', 'span'):                     # SPAN (Swift Parameter-free Attention Network): the published constructor surface
        cfg['type'] = 'span_net'
        cfg['num_in_ch'] = _pick(opts, 'in_nc', 3)
        cfg['num_out_ch'] = _pick(opts, 'out_nc', 3)
        cfg['feature_channels'] = _pick(opts, 'nf', 48)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['norm'] = _pick(opts, 'norm', True)
        cfg['deploy'] = _pick(opts, 'deploy', False)
    elif kind in ('realplksr', 'realplksr_net'):           # RealPLKSR (partial large-kernel conv, Mish, GroupNorm): the published constructor surface
        cfg['type'] = 'realplksr'
        cfg['in_ch'] = _pick(opts, 'in_nc', 3)
        cfg['out_ch'] = _pick(opts, 'out_nc', 3)
        cfg['dim'] = _pick(opts, 'nf', 64)
        cfg['n_blocks'] = _pick(opts, 'nb', 28)
        cfg['upscaling_factor'] = _pick(opts, 'scale', scale)
        cfg['kernel_size'] = _pick(opts, 'kernel_size', 17)
        cfg['split_ratio'] = _pick(opts, 'split_ratio', 0.25)
        cfg['use_ea'] = _pick(opts, 'use_ea', True)
        cfg['norm_groups'] = _pick(opts, 'norm_groups', 4)
    elif kind in ('swinir', 'swinir_net'):                 # SwinIR (window-attention transformer, the super-resolution forms): the published constructor surface
        cfg['type'] = 'swinir'
        cfg['in_chans'] = _pick(opts, 'in_nc', 3)
        cfg['embed_dim'] = _pick(opts, 'nf', 180)
        cfg['depths'] = list(_pick(opts, 'depths', [6] * 6))
        cfg['num_heads'] = list(_pick(opts, 'num_heads', [6] * len(cfg['depths'])))
        cfg['window_size'] = _pick(opts, 'window_size', 8)
        cfg['mlp_ratio'] = _pick(opts, 'mlp_ratio', 2.0)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['img_range'] = _pick(opts, 'img_range', 1.0)
        cfg['upsampler'] = _pick(opts, 'upsampler', 'pixelshuffle')
        cfg['resi_connection'] = _pick(opts, 'resi_connection', '1conv')
        opts.pop('out_nc', None)
    elif kind in ('swin2sr', 'swin2sr_net'):               # Swin2SR (SwinV2 blocks on SwinIR's skeleton): the published constructor surface
        cfg['type'] = 'swin2sr'
        cfg['in_chans'] = _pick(opts, 'in_nc', 3)
        cfg['embed_dim'] = _pick(opts, 'nf', 180)
        cfg['depths'] = list(_pick(opts, 'depths', [6] * 6))
        cfg['num_heads'] = list(_pick(opts, 'num_heads', [6] * len(cfg['depths'])))
        cfg['window_size'] = _pick(opts, 'window_size', 8)
        cfg['mlp_ratio'] = _pick(opts, 'mlp_ratio', 2.0)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['img_range'] = _pick(opts, 'img_range', 1.0)
        cfg['upsampler'] = _pick(opts, 'upsampler', 'pixelshuffle')
        cfg['resi_connection'] = _pick(opts, 'resi_connection', '1conv')
        cfg['cpb_hidden'] = _pick(opts, 'cpb_hidden', 512)           # (the width of cpb_mlp: 512 in the published code, read off the checkpoint)
        cfg['coords_table'] = _pick(opts, 'coords_table', None)      # the checkpoint's relative_coords_table, when it carries one
        opts.pop('out_nc', None)
    elif kind in ('hat', 'hat_net'):                       # HAT (hybrid attention transformer on SwinIR's skeleton): the published constructor surface
        cfg['type'] = 'hat'
        cfg['in_chans'] = _pick(opts, 'in_nc', 3)
        cfg['embed_dim'] = _pick(opts, 'nf', 180)
        cfg['depths'] = list(_pick(opts, 'depths', [6] * 6))
        cfg['num_heads'] = list(_pick(opts, 'num_heads', [6] * len(cfg['depths'])))
        cfg['window_size'] = _pick(opts, 'window_size', 16)
        cfg['compress_ratio'] = _pick(opts, 'compress_ratio', 3)
        cfg['squeeze_factor'] = _pick(opts, 'squeeze_factor', 30)
        cfg['conv_scale'] = _pick(opts, 'conv_scale', 0.01)          # (a constructor float no state dict carries: 0.01 in every published model)
        cfg['overlap_ratio'] = _pick(opts, 'overlap_ratio', 0.5)
        cfg['mlp_ratio'] = _pick(opts, 'mlp_ratio', 2.0)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['img_range'] = _pick(opts, 'img_range', 1.0)
        cfg['upsampler'] = _pick(opts, 'upsampler', 'pixelshuffle')
        cfg['resi_connection'] = _pick(opts, 'resi_connection', '1conv')
        cfg['rpi_sa'] = _pick(opts, 'rpi_sa', None)                  # the index buffers of the checkpoint, when it carries them
        cfg['rpi_oca'] = _pick(opts, 'rpi_oca', None)
        opts.pop('out_nc', None)
    elif kind in ('dat', 'dat_net'):                       # DAT (dual aggregation transformer on SwinIR's skeleton): the published constructor surface
        cfg['type'] = 'dat'
        cfg['in_chans'] = _pick(opts, 'in_nc', 3)
        cfg['embed_dim'] = _pick(opts, 'nf', 180)
        cfg['depth'] = list(_pick(opts, 'depths', [6] * 6))
        cfg['num_heads'] = list(_pick(opts, 'num_heads', [6] * len(cfg['depth'])))
        cfg['split_size'] = list(_pick(opts, 'split_size', [8, 32]))
        cfg['expansion_factor'] = _pick(opts, 'expansion_factor', 4.0)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['img_range'] = _pick(opts, 'img_range', 1.0)
        cfg['upsampler'] = _pick(opts, 'upsampler', 'pixelshuffle')
        cfg['resi_connection'] = _pick(opts, 'resi_connection', '1conv')
        cfg['pos_dim'] = _pick(opts, 'pos_dim', None)                # the width of the DynamicPosBias MLP, read off the checkpoint's pos_proj
        cfg['shift_blocks'] = _pick(opts, 'shift_blocks', None)      # [(group, block)] of the blocks that store attn_mask_0, when any does; else the published rule
        cfg['rpe_biases'] = _pick(opts, 'rpe_biases', None)          # the checkpoint's rpe_biases per branch, when it carries them
        cfg['split_assumed'] = _pick(opts, 'split_assumed', False)   # True: the checkpoint had no rpe_biases and [8, 32] was assumed
        opts.pop('out_nc', None)
    elif kind in ('drct', 'drct_net'):                     # DRCT (dense-residual Swin groups on SwinIR's skeleton): the published constructor surface
        cfg['type'] = 'drct'
        cfg['in_chans'] = _pick(opts, 'in_nc', 3)
        cfg['embed_dim'] = _pick(opts, 'nf', 180)
        cfg['depths'] = list(_pick(opts, 'depths', [6] * 6))
        cfg['num_heads'] = list(_pick(opts, 'num_heads', [6] * len(cfg['depths'])))
        cfg['window_size'] = _pick(opts, 'window_size', 16)
        cfg['mlp_ratio'] = _pick(opts, 'mlp_ratio', 2.0)
        cfg['upscale'] = _pick(opts, 'scale', scale)
        cfg['img_range'] = _pick(opts, 'img_range', 1.0)
        cfg['upsampler'] = _pick(opts, 'upsampler', 'pixelshuffle')
        cfg['resi_connection'] = _pick(opts, 'resi_connection', '1conv')
        cfg['gc'] = _pick(opts, 'gc', 32)
        cfg['block_heads'] = _pick(opts, 'block_heads', None)        # per block, read off the checkpoint's bias tables (None: the published rule)
        cfg['block_hidden'] = _pick(opts, 'block_hidden', None)      # per block, read off mlp.fc1 (None: int(dim mlp_ratio))
        opts.pop('out_nc', None)
    else:
        raise NotImplementedError(f'Generator model [{kind:s}] not recognized')

    if opts:            # the reference prints unprocessed options (defaults.py:145-146)
        print(opts)
    return cfg
