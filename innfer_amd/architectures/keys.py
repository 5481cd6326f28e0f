"""State-dict key -> shape tables of the reference generators (host logic, no torch).

The nn.Module shells in this package are built FROM these tables, so their
state_dict() keys are the reference's by construction and model-database .pth
files load with strict=True.
"""


def _bn(s, key, c):
    s[key + ".weight"] = (c,); s[key + ".bias"] = (c,)
    s[key + ".running_mean"] = (c,); s[key + ".running_var"] = (c,); s[key + ".num_batches_tracked"] = ()


def rrdbnet_shapes(in_nc=3, out_nc=3, nf=64, nb=23, gc=32, scale=4, plus=False, nr=3, upsample_mode='upconv', norm=False, mode='CNA'):
    """State-dict key -> shape of the reference's old-arch ESRGAN
    (reference RRDBNet_arch.py:16-48; key layout SURVEY.md 3.3).  nr != 3: the dense blocks are `RDBs.<i>` (RRDBNet_arch.py:84-88);
    upsample_mode 'pixelshuffle': the stage's conv (nf -> 4 nf, 9 nf for scale 3) comes first (block.py:333-346)."""
    import math
    s = {"model.0.weight": (nf, in_nc, 3, 3), "model.0.bias": (nf,)}
    for b in range(nb):
        for r in range(1, nr + 1):
            p = f"model.1.sub.{b}.RDB{r}." if nr == 3 else f"model.1.sub.{b}.RDBs.{r - 1}."
            if plus:
                s[p + "conv1x1.weight"] = (gc, nf, 1, 1)
            for i in range(1, 6):
                cin = nf + (i - 1) * gc
                cout = gc if i < 5 else nf
                s[p + f"conv{i}.0.weight"] = (cout, cin, 3, 3)
                s[p + f"conv{i}.0.bias"] = (cout,)
                if norm:                        # conv_block(CNA) = conv, BatchNorm2d[, act] (block.py:244-246)
                    _bn(s, p + f"conv{i}.1", cout)
    lr = nb
    if norm and mode == 'NAC':                  # LR_conv = norm, conv (block.py:246-254): the norm layer takes the conv's slot, the conv the next
        _bn(s, f"model.1.sub.{nb}", nf)
        lr = nb + 1
    s[f"model.1.sub.{lr}.weight"] = (nf, nf, 3, 3)
    s[f"model.1.sub.{lr}.bias"] = (nf,)
    if norm and mode != 'NAC':                  # LR_conv's norm layer is flattened into the trunk's Sequential behind its conv
        _bn(s, f"model.1.sub.{nb + 1}", nf)
    n_up = 1 if scale == 3 else int(math.log(scale, 2))
    idx = 2
    for _ in range(n_up):
        if upsample_mode == 'pixelshuffle':
            f = 9 if scale == 3 else 4
            s[f"model.{idx}.weight"] = (nf * f, nf, 3, 3)
            s[f"model.{idx}.bias"] = (nf * f,)
        else:
            s[f"model.{idx + 1}.weight"] = (nf, nf, 3, 3)
            s[f"model.{idx + 1}.bias"] = (nf,)
        idx += 3
    s[f"model.{idx}.weight"] = (nf, nf, 3, 3)
    s[f"model.{idx}.bias"] = (nf,)
    s[f"model.{idx + 2}.weight"] = (out_nc, nf, 3, 3)
    s[f"model.{idx + 2}.bias"] = (out_nc,)
    return s


def mrrdbnet_shapes(in_nc=3, out_nc=3, nf=64, nb=24, gc=32):
    """State-dict key -> shape of the modified ("new"-arch) ESRGAN, MRRDBNet (reference RRDBNet_arch.py:173-231):
    the graph of the old-arch 4x RRDBNet under different names."""
    s = {"conv_first.weight": (nf, in_nc, 3, 3), "conv_first.bias": (nf,)}
    for b in range(nb):
        for r in (1, 2, 3):
            for i in range(1, 6):
                cin = nf + (i - 1) * gc
                cout = gc if i < 5 else nf
                s[f"RRDB_trunk.{b}.RDB{r}.conv{i}.weight"] = (cout, cin, 3, 3)
                s[f"RRDB_trunk.{b}.RDB{r}.conv{i}.bias"] = (cout,)
    for name in ("trunk_conv", "upconv1", "upconv2", "HRconv"):
        s[name + ".weight"] = (nf, nf, 3, 3)
        s[name + ".bias"] = (nf,)
    s["conv_last.weight"] = (out_nc, nf, 3, 3)
    s["conv_last.bias"] = (out_nc,)
    return s


def mrrdb_key_of(old_key, nb):
    """Old-arch conv key of the engine ('model.1.sub.3.RDB2.conv4.0') -> MRRDBNet's name for the same conv
    (the inverse of mod2normal, utils.py:666-698, for any nb)."""
    fixed = {"model.0": "conv_first", f"model.1.sub.{nb}": "trunk_conv", "model.3": "upconv1",
             "model.6": "upconv2", "model.8": "HRconv", "model.10": "conv_last"}
    if old_key in fixed:
        return fixed[old_key]
    assert old_key.startswith("model.1.sub.") and old_key.endswith(".0"), old_key
    return "RRDB_trunk." + old_key[len("model.1.sub."):-2]


# BasicSR's RRDBNet (rrdbnet_arch.py; the Real-ESRGAN releases): its fixed conv names -> the engine's old-arch names for the same convs.  THE table: the
# names are BasicSR's as published; a correction goes here and nowhere else.  '{nb}' is the number of blocks.
REALESRGAN_FIXED = (
    ("conv_first", "model.0"),
    ("conv_body", "model.1.sub.{nb}"),
    ("conv_up1", "model.3"),
    ("conv_up2", "model.6"),
    ("conv_hr", "model.8"),
    ("conv_last", "model.10"),
)
# a dense-block conv: BasicSR 'body.<b>.rdb<m>.conv<k>' <-> old-arch 'model.1.sub.<b>.RDB<m>.conv<k>.0'
REALESRGAN_BLOCK = ("body.{b}.rdb{m}.conv{k}", "model.1.sub.{b}.RDB{m}.conv{k}.0")
REALESRGAN_UNSHUFFLE = {4: 1, 2: 2, 1: 4}          # BasicSR `scale` -> pixel_unshuffle factor in front of conv_first (the graph behind it is always the 4x one)


def realesrgan_key_map(nb):
    """{BasicSR conv prefix: old-arch conv prefix} of an nb-block BasicSR RRDBNet ('.weight' / '.bias' follow both)."""
    m = {new: old.format(nb=nb) for new, old in REALESRGAN_FIXED}
    for b in range(nb):
        for r in (1, 2, 3):
            for k in range(1, 6):
                m[REALESRGAN_BLOCK[0].format(b=b, m=r, k=k)] = REALESRGAN_BLOCK[1].format(b=b, m=r, k=k)
    return m


def realesrgan_key_of(old_key, nb):
    """Old-arch conv key of the engine -> BasicSR's name for the same conv."""
    inv = {old: new for new, old in realesrgan_key_map(nb).items()}
    return inv[old_key]


def realesrgan_shapes(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
    """State-dict key -> shape of BasicSR's RRDBNet: the old-arch 4x graph under BasicSR's names, conv_first taking num_in_ch * r^2 channels
    (r = 1, 2, 4 for scale 4, 2, 1: pixel_unshuffle in front of it)."""
    r = REALESRGAN_UNSHUFFLE[scale]
    old = rrdbnet_shapes(num_in_ch * r * r, num_out_ch, num_feat, num_block, num_grow_ch, 4)
    s = {}
    for new, o in realesrgan_key_map(num_block).items():
        s[new + ".weight"] = old[o + ".weight"]
        s[new + ".bias"] = old[o + ".bias"]
    return s


def compact_shapes(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type='prelu'):
    """State-dict key -> shape of BasicSR's SRVGGNetCompact (realesr-animevideov3, realesr-general-x4v3, the "compact" community models): `body`, a ModuleList
    of 2 num_conv + 3 entries -- body.0 the first conv, body.2i (i = 1 .. num_conv) the nf -> nf convs, each followed by its activation at the next index
    (a PReLU(num_feat) carries `weight` [num_feat]; ReLU / LeakyReLU carry nothing), body.<2 num_conv + 2> the last conv to num_out_ch * upscale^2 channels."""
    s = {}
    cin = num_in_ch
    for i in range(num_conv + 1):
        s[f"body.{2 * i}.weight"] = (num_feat, cin, 3, 3)
        s[f"body.{2 * i}.bias"] = (num_feat,)
        if act_type == 'prelu':
            s[f"body.{2 * i + 1}.weight"] = (num_feat,)
        cin = num_feat
    last = 2 * num_conv + 2
    s[f"body.{last}.weight"] = (num_out_ch * upscale * upscale, num_feat, 3, 3)
    s[f"body.{last}.bias"] = (num_out_ch * upscale * upscale,)
    return s


def span_convs():
    """Prefixes of SPAN's thirteen Conv3XC units in forward order: conv_1, block_<i>.c<j>_r (i = 1 .. 6, j = 1 .. 3), conv_2."""
    return ['conv_1'] + [f'block_{i}.c{j}_r' for i in range(1, 7) for j in range(1, 4)] + ['conv_2']


def span_shapes(num_in_ch=3, num_out_ch=3, feature_channels=48, upscale=4, norm=True, deploy=False, gain=2):
    """State-dict key -> shape of SPAN (Swift Parameter-free Attention Network).  Conv3XC(ci, co, gain) carries sk = Conv2d(ci, co, 1), conv.0 = Conv2d(ci, ci gain, 1),
    conv.1 = Conv2d(ci gain, co gain, 3), conv.2 = Conv2d(co gain, co, 1) and eval_conv = Conv2d(ci, co, 3) -- a `deploy` checkpoint only eval_conv; then
    conv_cat = Conv2d(4 f, f, 1) and upsampler.0 = Conv2d(f, num_out_ch upscale^2, 3).  norm=False checkpoints carry a one-element buffer `no_norm`."""
    f = feature_channels
    s = {}

    def conv(k, co, ci, ks):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)
    for p in span_convs():
        ci = num_in_ch if p == 'conv_1' else f
        if not deploy:
            conv(p + '.sk', f, ci, 1)
            conv(p + '.conv.0', ci * gain, ci, 1)
            conv(p + '.conv.1', f * gain, ci * gain, 3)
            conv(p + '.conv.2', f, f * gain, 1)
        conv(p + '.eval_conv', f, ci, 3)
    conv('conv_cat', f, 4 * f, 1)
    conv('upsampler.0', num_out_ch * upscale * upscale, f, 3)
    if not norm:
        s['no_norm'] = (1,)
    return s


def realplksr_shapes(in_ch=3, out_ch=3, dim=64, n_blocks=28, upscaling_factor=4, kernel_size=17, split_ratio=0.25, use_ea=True):
    """State-dict key -> shape of RealPLKSR: feats.0 = Conv2d(in_ch, dim, 3); feats.<i> (i = 1 .. n_blocks) a PLKBlock -- channel_mixer.0 = Conv2d(dim, 2 dim, 3),
    channel_mixer.2 = Conv2d(2 dim, dim, 3), lk.conv = Conv2d(p, p, k) with p = int(dim split_ratio), attn.f.0 = Conv2d(dim, dim, 3) (only with use_ea),
    refine = Conv2d(dim, dim, 1), norm = GroupNorm(norm_groups, dim) --; feats.<n_blocks + 1> is a Dropout2d (no keys); feats.<n_blocks + 2> =
    Conv2d(dim, out_ch upscaling_factor^2, 3).  norm_groups leaves no trace in the keys."""
    p = int(dim * split_ratio)
    s = {}

    def conv(k, co, ci, ks):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)
    conv('feats.0', dim, in_ch, 3)
    for i in range(1, n_blocks + 1):
        conv(f'feats.{i}.channel_mixer.0', 2 * dim, dim, 3)
        conv(f'feats.{i}.channel_mixer.2', dim, 2 * dim, 3)
        conv(f'feats.{i}.lk.conv', p, p, kernel_size)
        if use_ea:
            conv(f'feats.{i}.attn.f.0', dim, dim, 3)
        conv(f'feats.{i}.refine', dim, dim, 1)
        s[f'feats.{i}.norm.weight'], s[f'feats.{i}.norm.bias'] = (dim,), (dim,)
    conv(f'feats.{n_blocks + 2}', out_ch * upscaling_factor ** 2, dim, 3)
    return s


def swinir_shapes(in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=6, mlp_ratio=2.0, upscale=4, upsampler='pixelshuffle', resi_connection='1conv', window_size=8):
    """State-dict key -> shape of the PARAMETERS of SwinIR (KAIR / BasicSR swinir_arch.py; patch_size 1, qkv_bias, patch_norm, no absolute position embedding).  The buffers
    (attn.relative_position_index on every block, attn_mask on the odd ones) are not parameters: the index is a formula and the mask depends on img_size."""
    C, hid, s = embed_dim, int(embed_dim * mlp_ratio + 1e-6), {}

    def lin(k, co, ci):
        s[k + '.weight'], s[k + '.bias'] = (co, ci), (co,)

    def conv(k, co, ci, ks=3):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)

    def norm(k):
        s[k + '.weight'], s[k + '.bias'] = (C,), (C,)

    def resi(k):
        if resi_connection == '3conv':
            conv(k + '.0', C // 4, C); conv(k + '.2', C // 4, C // 4, 1); conv(k + '.4', C, C // 4)
        else:
            conv(k, C, C)
    conv('conv_first', C, in_chans)
    norm('patch_embed.norm')
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f'layers.{i}.residual_group.blocks.{j}.'
            norm(b + 'norm1')
            s[b + 'attn.relative_position_bias_table'] = ((2 * window_size - 1) ** 2, num_heads)
            lin(b + 'attn.qkv', 3 * C, C)
            lin(b + 'attn.proj', C, C)
            norm(b + 'norm2')
            lin(b + 'mlp.fc1', hid, C)
            lin(b + 'mlp.fc2', C, hid)
        resi(f'layers.{i}.conv')
    norm('norm')
    resi('conv_after_body')
    if upsampler == 'pixelshuffledirect':
        conv('upsample.0', upscale * upscale * in_chans, C)
        return s
    conv('conv_before_upsample.0', 64, C)
    if upsampler == 'pixelshuffle':
        if upscale == 3:
            conv('upsample.0', 576, 64)
        else:
            for st in range(max(1, upscale.bit_length() - 1)):
                conv(f'upsample.{2 * st}', 256, 64)
    else:                                    # nearest+conv
        conv('conv_up1', 64, 64)
        if upscale == 4:
            conv('conv_up2', 64, 64)
        conv('conv_hr', 64, 64)
    conv('conv_last', in_chans, 64)
    return s


def swin2sr_shapes(in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=6, mlp_ratio=2.0, upscale=4, upsampler='pixelshuffle', resi_connection='1conv', window_size=8,
                   cpb_hidden=512):
    """State-dict key -> shape of the PARAMETERS of Swin2SR (the published network_swin2sr.py; patch_size 1, qkv_bias, patch_norm, no absolute position embedding): SwinIR's
    keys with another attention -- no relative_position_bias_table and no qkv.bias; logit_scale, the continuous-position-bias MLP, q_bias and v_bias instead.  The buffers
    (attn.relative_coords_table and attn.relative_position_index on every block, attn_mask on the odd ones) are not parameters."""
    s = {}
    for k, shp in swinir_shapes(in_chans, embed_dim, depths, num_heads, mlp_ratio, upscale, upsampler, resi_connection, window_size).items():
        if k.endswith('attn.relative_position_bias_table'):
            a = k[:-len('relative_position_bias_table')]
            s[a + 'logit_scale'] = (num_heads, 1, 1)
            s[a + 'cpb_mlp.0.weight'], s[a + 'cpb_mlp.0.bias'], s[a + 'cpb_mlp.2.weight'] = (cpb_hidden, 2), (cpb_hidden,), (num_heads, cpb_hidden)
            s[a + 'q_bias'], s[a + 'v_bias'] = (embed_dim,), (embed_dim,)
        elif not k.endswith('attn.qkv.bias'):
            s[k] = shp
    return s


def hat_shapes(in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=6, mlp_ratio=2.0, upscale=4, compress_ratio=3, squeeze_factor=30, window_size=16,
               overlap_win_size=24):
    """State-dict key -> shape of the PARAMETERS of HAT (the published hat_arch.py; patch_size 1, qkv_bias, patch_norm, no absolute position embedding, the pixelshuffle
    tail, '1conv').  The two top-level buffers (relative_position_index_SA / _OCA) are not parameters."""
    C, hid, s = embed_dim, int(embed_dim * mlp_ratio + 1e-6), {}

    def lin(k, co, ci):
        s[k + '.weight'], s[k + '.bias'] = (co, ci), (co,)

    def conv(k, co, ci, ks=3):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)

    def norm(k):
        s[k + '.weight'], s[k + '.bias'] = (C,), (C,)
    conv('conv_first', C, in_chans)
    norm('patch_embed.norm')
    for i, depth in enumerate(depths):
        g = f'layers.{i}.residual_group.'
        for j in range(depth):
            b = g + f'blocks.{j}.'
            norm(b + 'norm1')
            s[b + 'attn.relative_position_bias_table'] = ((2 * window_size - 1) ** 2, num_heads)
            lin(b + 'attn.qkv', 3 * C, C)
            lin(b + 'attn.proj', C, C)
            conv(b + 'conv_block.cab.0', C // compress_ratio, C)
            conv(b + 'conv_block.cab.2', C, C // compress_ratio)
            conv(b + 'conv_block.cab.3.attention.1', C // squeeze_factor, C, 1)
            conv(b + 'conv_block.cab.3.attention.3', C, C // squeeze_factor, 1)
            norm(b + 'norm2')
            lin(b + 'mlp.fc1', hid, C)
            lin(b + 'mlp.fc2', C, hid)
        o = g + 'overlap_attn.'
        norm(o + 'norm1')
        s[o + 'relative_position_bias_table'] = ((window_size + overlap_win_size - 1) ** 2, num_heads)
        lin(o + 'qkv', 3 * C, C)
        lin(o + 'proj', C, C)
        norm(o + 'norm2')
        lin(o + 'mlp.fc1', hid, C)
        lin(o + 'mlp.fc2', C, hid)
        conv(f'layers.{i}.conv', C, C)
    norm('norm')
    conv('conv_after_body', C, C)
    conv('conv_before_upsample.0', 64, C)
    if upscale == 3:
        conv('upsample.0', 576, 64)
    else:
        for st in range(max(1, upscale.bit_length() - 1)):
            conv(f'upsample.{2 * st}', 256, 64)
    conv('conv_last', in_chans, 64)
    return s


DRCT_GC = 32        # the dense group's growth: every adjust conv but the last makes 32 channels


def drct_head_rule(dim, num_heads):
    """Heads of a DRCT Swin block on `dim` channels as the published code is recalled to choose them: num_heads - (dim % num_heads).  Only a cross-check and the default of
    the shell: a checkpoint's relative_position_bias_table.shape[1] decides."""
    return num_heads - dim % num_heads


def drct_shapes(in_chans=3, embed_dim=180, n_groups=6, num_heads=6, mlp_ratio=2.0, upscale=4, block_heads=None, block_hidden=None):
    """State-dict key -> shape of the PARAMETERS of DRCT (the published drct_arch.py, written down without the source at hand; patch_size 1, qkv_bias, patch_norm, no absolute
    position embedding, gc 32, the pixelshuffle tail).  THE ONE PLACE a correction of a key name or a shape goes: the shell, the loader, the synthetic checkpoints and the
    tests are built from this table.  block_heads / block_hidden: per block, 5 n_groups entries (block k of group g at 5 g + k), as a checkpoint states them; None: the
    published rule and int(dim mlp_ratio).  Not in it, because they are buffers: attn.relative_position_index of every block, attn_mask of the shifted ones."""
    C, s = embed_dim, {}

    def lin(k, co, ci):
        s[k + '.weight'], s[k + '.bias'] = (co, ci), (co,)

    def conv(k, co, ci, ks=3):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)

    def norm(k, c=C):
        s[k + '.weight'], s[k + '.bias'] = (c,), (c,)
    conv('conv_first', C, in_chans)
    norm('patch_embed.norm')
    for i in range(n_groups):
        for k in range(5):
            dim = C + DRCT_GC * k
            nh = drct_head_rule(dim, num_heads) if block_heads is None else block_heads[5 * i + k]
            hid = int(dim * mlp_ratio + 1e-6) if block_hidden is None else block_hidden[5 * i + k]
            b = f'layers.{i}.swin{k + 1}.'
            norm(b + 'norm1', dim)
            s[b + 'attn.relative_position_bias_table'] = (961, nh)
            lin(b + 'attn.qkv', 3 * dim, dim)
            lin(b + 'attn.proj', dim, dim)
            norm(b + 'norm2', dim)
            lin(b + 'mlp.fc1', hid, dim)
            lin(b + 'mlp.fc2', dim, hid)
            conv(f'layers.{i}.adjust{k + 1}', DRCT_GC if k < 4 else C, dim, 1)
    norm('norm')
    conv('conv_after_body', C, C)
    conv('conv_before_upsample.0', 64, C)
    if upscale == 3:
        conv('upsample.0', 576, 64)
    else:
        for st in range(max(1, upscale.bit_length() - 1)):
            conv(f'upsample.{2 * st}', 256, 64)
    conv('conv_last', in_chans, 64)
    return s


def dat_pos_dim(embed_dim):
    """Width of the DynamicPosBias MLP of a DAT branch as recalled from the published code (the branch's dim // 4, again // 4); a checkpoint's pos_proj.weight decides."""
    return ((embed_dim // 2) // 4) // 4


def dat_shapes(in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=6, expansion_factor=4.0, upscale=4, upsampler='pixelshuffle', resi_connection='1conv',
               pos_dim=None):
    """State-dict key -> shape of the PARAMETERS (and BatchNorm statistics) of DAT (the published dat_arch.py, written down without the source at hand).  THE ONE PLACE a
    correction of a key name or a shape goes: the shell, the loader, the synthetic checkpoints and the tests' reference are all built from this table.  Not in it, because
    they are buffers: attn.attns.<0|1>.rpe_biases, attn.attns.<0|1>.relative_position_index and, on shifted blocks, attn.attn_mask_0 / _1."""
    C, nH, s = embed_dim, num_heads, {}
    hid = int(C * expansion_factor)
    p = dat_pos_dim(C) if pos_dim is None else pos_dim

    def lin(k, co, ci):
        s[k + '.weight'], s[k + '.bias'] = (co, ci), (co,)

    def conv(k, co, ci, ks=3):
        s[k + '.weight'], s[k + '.bias'] = (co, ci, ks, ks), (co,)

    def norm(k, c=C):
        s[k + '.weight'], s[k + '.bias'] = (c,), (c,)

    def resi(k):
        if resi_connection == '3conv':
            conv(k + '.0', C // 4, C); conv(k + '.2', C // 4, C // 4, 1); conv(k + '.4', C, C // 4)
        else:
            conv(k, C, C)
    conv('conv_first', C, in_chans)
    norm('before_RG.1')
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f'layers.{i}.blocks.{j}.'
            norm(b + 'norm1')
            lin(b + 'attn.qkv', 3 * C, C)
            lin(b + 'attn.proj', C, C)
            conv(b + 'attn.dwconv.0', C, 1)                          # depthwise: groups = C
            _bn(s, b + 'attn.dwconv.1', C)
            conv(b + 'attn.channel_interaction.1', C // 8, C, 1)
            _bn(s, b + 'attn.channel_interaction.2', C // 8)
            conv(b + 'attn.channel_interaction.4', C, C // 8, 1)
            conv(b + 'attn.spatial_interaction.0', C // 16, C, 1)
            _bn(s, b + 'attn.spatial_interaction.1', C // 16)
            conv(b + 'attn.spatial_interaction.3', 1, C // 16, 1)
            if j % 2 == 0:
                for br in (0, 1):
                    a = b + f'attn.attns.{br}.pos.'
                    lin(a + 'pos_proj', p, 2)
                    for m in ('pos1', 'pos2'):
                        norm(a + m + '.0', p); lin(a + m + '.2', p, p)
                    norm(a + 'pos3.0', p); lin(a + 'pos3.2', nH // 2, p)
            else:
                s[b + 'attn.temperature'] = (nH, 1, 1)
            norm(b + 'norm2')
            lin(b + 'ffn.fc1', hid, C)
            norm(b + 'ffn.sg.norm', hid // 2)
            conv(b + 'ffn.sg.conv', hid // 2, 1)                     # depthwise: groups = hid / 2
            lin(b + 'ffn.fc2', C, hid // 2)
        resi(f'layers.{i}.conv')
    norm('norm')
    resi('conv_after_body')
    if upsampler == 'pixelshuffledirect':
        conv('upsample.0', upscale * upscale * in_chans, C)
        return s
    conv('conv_before_upsample.0', 64, C)
    if upscale == 3:
        conv('upsample.0', 576, 64)
    else:
        for st in range(max(1, upscale.bit_length() - 1)):
            conv(f'upsample.{2 * st}', 256, 64)
    conv('conv_last', in_chans, 64)
    return s


def srresnet_layout(nb, norm=False, mode='CNA'):
    """Positions of a ResNetBlock's / LR_conv's layers inside the flattened Sequentials (SRResNet_arch.py:23-27,68-86; block.py:242-254,
    B.sequential flattens nested Sequentials): {engine key -> (conv key, BatchNorm in front of the conv or None, BatchNorm behind it or None)}.
    Engine keys are the default graph's (norm none, CNA): `model.1.sub.<b>.res.0`, `.res.2`, `model.1.sub.<nb>`."""
    lay = {}
    for b in range(nb):
        p = f"model.1.sub.{b}.res."
        if mode == 'NAC':            # [norm,] act, conv, [norm,] act, conv
            if norm: lay[p + "0"], lay[p + "2"] = (p + "2", p + "0", p + "3"), (p + "5", None, None)     # the 2nd block's norm follows conv0: folded there
            else: lay[p + "0"], lay[p + "2"] = (p + "1", None, None), (p + "3", None, None)
        elif mode == 'CNAC':         # conv, [norm,] act, conv
            if norm: lay[p + "0"], lay[p + "2"] = (p + "0", None, p + "1"), (p + "3", None, None)
            else: lay[p + "0"], lay[p + "2"] = (p + "0", None, None), (p + "2", None, None)
        else:                        # conv, [norm,] act, conv[, norm]
            if norm: lay[p + "0"], lay[p + "2"] = (p + "0", None, p + "1"), (p + "3", None, p + "4")
            else: lay[p + "0"], lay[p + "2"] = (p + "0", None, None), (p + "2", None, None)
    lr = f"model.1.sub.{nb}"
    if not norm: lay[lr] = (lr, None, None)
    elif mode == 'NAC': lay[lr] = (f"model.1.sub.{nb + 1}", lr, None)
    else: lay[lr] = (lr, None, f"model.1.sub.{nb + 1}")
    return lay


def srresnet_shapes(in_nc=3, out_nc=3, nf=64, nb=16, scale=4, upsample_mode='pixelshuffle', norm=False, mode='CNA'):
    """SRGAN/SRResNet keys (reference SRResNet_arch.py:15-46, defaults.py:53-67); upsample_mode 'upconv': Upsample, conv, act per stage;
    norm / mode: BatchNorm2d layers and the layer order of the conv blocks (srresnet_layout)."""
    import math
    s = {"model.0.weight": (nf, in_nc, 3, 3), "model.0.bias": (nf,)}
    lay = srresnet_layout(nb, norm, mode)
    ordered = [f"model.1.sub.{b}.res.{j}" for b in range(nb) for j in (0, 2)] + [f"model.1.sub.{nb}"]
    for ek in ordered:
        conv, pre, post = lay[ek]
        if pre: _bn(s, pre, nf)
        s[conv + ".weight"] = (nf, nf, 3, 3)
        s[conv + ".bias"] = (nf,)
        if post: _bn(s, post, nf)
    n_up = 1 if scale == 3 else int(math.log(scale, 2))
    idx = 2
    for _ in range(n_up):
        if upsample_mode == 'upconv':
            s[f"model.{idx + 1}.weight"] = (nf, nf, 3, 3)
            s[f"model.{idx + 1}.bias"] = (nf,)
        else:
            s[f"model.{idx}.weight"] = (nf * (9 if scale == 3 else 4), nf, 3, 3)
            s[f"model.{idx}.bias"] = (nf * (9 if scale == 3 else 4),)
        idx += 3
    s[f"model.{idx}.weight"] = (nf, nf, 3, 3)
    s[f"model.{idx}.bias"] = (nf,)
    s[f"model.{idx + 2}.weight"] = (out_nc, nf, 3, 3)
    s[f"model.{idx + 2}.bias"] = (out_nc,)
    return s
