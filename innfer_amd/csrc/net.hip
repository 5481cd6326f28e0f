// Network engine: RRDBNet (ESRGAN) and SRResNet (SRGAN) forward as a sequence of
// fused conv launches over fp16 blocked-NHWC channel slabs ([C/32][N*H*W][32]) in a caller-provided workspace.
//
// Replaces the nn.Sequential graph of RRDBNet_arch.py:16-62 / SRResNet_arch.py:15-91:
//   torch.cat            -> channel-group offsets inside a 6-group slab (x|x|x1|x2|x3|x4)
//   LeakyReLU / ReLU     -> conv epilogue
//   x5*0.2 + x, RRDB out*0.2 + x, ShortcutBlock x + sub(x) -> conv epilogue
//   Upsample(nearest 2x) -> folded into the next conv's input addressing
//   PixelShuffle(2)      -> folded into the conv's store
#include "common.h"
#include "norm_stats.h"
#include "test_entry.h"

#include <cmath>
#include <cstring>
#include <mutex>

namespace innfer {

static thread_local std::string g_err;

int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {
struct GtRec { std::string name; hipEvent_t e0, e1; double flops, bytes; };
thread_local std::vector<GtRec>* g_gt = nullptr;
thread_local hipEvent_t g_gt_e0 = nullptr;
}  // namespace
bool gt_on() { return g_gt != nullptr; }
void gt_begin(hipStream_t s) {
    if (!g_gt) return;
    g_gt_e0 = nullptr;
    if (hipEventCreate(&g_gt_e0) != hipSuccess || hipEventRecord(g_gt_e0, s) != hipSuccess) g_gt_e0 = nullptr;
}
void gt_end(hipStream_t s, const char* name, double flops, double bytes) {
    if (!g_gt || !g_gt_e0) return;
    hipEvent_t e1 = nullptr;
    if (hipEventCreate(&e1) != hipSuccess || hipEventRecord(e1, s) != hipSuccess) return;
    g_gt->push_back(GtRec{name, g_gt_e0, e1, flops, bytes});
    g_gt_e0 = nullptr;
}

}  // namespace innfer

using namespace innfer;

extern "C" int innfer_timer_start(void) {
    if (g_gt) return set_error(INNFER_ERR_INVALID, "timer_start: a collection is already open on this thread");
    g_gt = new std::vector<GtRec>();
    return INNFER_OK;
}

extern "C" int innfer_timer_stop(void* stream, int cap, char* names, int name_cap, float* ms, double* flops, double* bytes, int* n) {
    if (!g_gt) return set_error(INNFER_ERR_INVALID, "timer_stop: no collection is open on this thread");
    std::vector<GtRec>* recs = g_gt;
    g_gt = nullptr;
    int rc = INNFER_OK;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = set_error(INNFER_ERR_HIP, "timer_stop: stream synchronize failed");
    if (n) *n = (int)recs->size();
    for (int i = 0; i < (int)recs->size(); ++i) {
        GtRec& r = (*recs)[i];
        if (rc == INNFER_OK && i < cap) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, r.e0, r.e1);
            if (ms) ms[i] = t;
            if (flops) flops[i] = r.flops;
            if (bytes) bytes[i] = r.bytes;
            if (names && name_cap > 0) { strncpy(names + (size_t)i * name_cap, r.name.c_str(), name_cap - 1); names[(size_t)i * name_cap + name_cap - 1] = 0; }
        }
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    delete recs;
    return rc;
}

struct ConvSlot {
    std::string key;
    int K = 0, C = 0;
    bool first = false;          // the network's first conv: first_conv_mfma, few input channels (fp32 [C*9][K] weights, first_conv_layout)
    int ksize = 3;               // 1: a 1x1 conv (one-tap panel, ConvLaunch.conv1x1)
    void* d_w = nullptr;         // packed panels (MFMA) or fp32 k-major (first)
    std::vector<float> h_w;      // MFMA convs: the fp32 weights as they were set, kept for the fp32-accurate mode's panels
    void* d_w32 = nullptr;       //   (hi | lo | hi) panels of conv_pack_split, built by innfer_net_set_precision(1)
    bool rowp = false;           // 3x3 convs of exactly 64 outputs: d_w (and d_up4, d_fuse behind it) in the plane row order (ConvLaunch.rowp) -- a store instruction of the 64-channel
                                 // kernels then touches one slab plane; set when the weights are packed.  The split panels (d_w32) keep the lane-contiguous order.
    bool up2x = false;           // the conv of an upconv_block (nearest 2x in front of it): also packed as the four 2x2-tap phases of the equivalent transposed conv
    void* d_up4 = nullptr;       //   conv_pack_deconv2x panels of the summed weights + d_b4 (the bias once per phase), built with d_w
    void* d_up4p = nullptr;      //   the same in the plane row order (rowp slots: the one-visit form, conv3x3_pc UP4); d_up4 stays lane-contiguous (grids <= 16 wide, A/B)
    float* d_b4 = nullptr;
    bool ps2 = false;            // the conv in front of a PixelShuffle(2) stage (nf -> 4 nf, nf 64): also packed phase-major in the plane row order (conv_pack_shuffle2)
    void* d_ps = nullptr;        //   those panels + d_bps (the bias in the same order): the shuffle is the producer / consumer kernel's store (ConvLaunch.rowp = 2)
    float* d_bps = nullptr;
    void* d_fuse = nullptr;      // a last conv of 64 -> <= 3 channels: its panel for the epilogue of HR_conv0 (conv_pack_fuse_last), built with d_w
    float* d_b = nullptr;        // bias padded to the panel width
    int Kp = 0;                  // SRVGGNetCompact's last conv (K = out_nc * scale^2 = 1 .. 64): the width of the zero-padded panel it runs on as a slab conv, 32 or 64
    bool slope_ok = false;       // SRVGGNetCompact's activated convs: the conv's epilogue is act 8 with the per-channel slopes of innfer_net_set_conv_slope
    float* d_slope = nullptr;    //   those slopes, padded with zeros like d_b
    bool loaded = false;
    // mode 'NAC' conv blocks (block.py:246-254: norm -> act -> conv): the conv reads act(alpha[c] * x + shift[c]); an elementwise pass in front of it
    bool map_ok = false;         // slot may carry an input map (first conv of an SRResNet block, LR_conv)
    float* d_map = nullptr;      // alpha[C] then shift[C]
    int map_act = 0;
    // RealPLKSR (kind 4)
    bool plk = false;            // lk.conv: [16, 16, k, k] on csrc/plk_conv.hip (ksize = k; d_w: plk_pack panel, d_b: 16 floats)
    bool lane_rows = false;      // attn.f.0: a 64-output conv whose epilogue is the gate act 5 -- a form of the lane-contiguous panels only, so d_w is never packed in the plane row order
    bool gn_ok = false;          // refine: GroupNorm(groups, 64) follows it -- d_gn: gamma[64] then beta[64] (innfer_net_set_group_norm)
    float* d_gn = nullptr;
    // SwinIR (kind 5)
    float mult = 1.f;            // pixels this conv runs on per pixel of the padded LR grid (the tail's convs behind an upsampling stage): innfer_net_flops
};

struct innfer_net {
    int kind = 0;                // 0 rrdbnet, 1 srresnet, 2 BasicSR's SRVGGNetCompact (innfer_compact_create; compact_forward), 3 SPAN (innfer_span_create; span_forward), 4 RealPLKSR (innfer_plksr_create; plksr_forward)
    int plk_k = 17, plk_ea = 1, plk_groups = 4;      // RealPLKSR: kernel_size, use_ea, norm_groups
    // SwinIR (kind 5; innfer_swinir_create): C = embed_dim padded to sw_cp, sw_nh heads of sw_d channels, the MLP's hidden size padded to sw_hp, RSTB depths, the tail
    // (0 pixelshuffle, 1 pixelshuffledirect, 2 nearest+conv), resi_connection '3conv' (C / 4 padded to sw_c4p); the LayerNorm parameters (gamma[C] then beta[C] per norm, in
    // the order patch_embed.norm, (norm1, norm2) per block, norm) and the dense relative position bias of every block ([nH][64][64])
    int sw_c = 0, sw_cp = 0, sw_nh = 0, sw_d = 0, sw_hid = 0, sw_hp = 0, sw_tail = 0, sw_conv3 = 0, sw_c4p = 0;
    std::vector<int> sw_depths;
    std::vector<float*> sw_ln, sw_relb;
    // HAT (kind 6; innfer_hat_create) on SwinIR's fields: 16 x 16 windows; per HAB the conv block's two 3x3 convs (C -> hat_cc <= 64 -> C) and its channel attention
    // (hat_ca[blk]: W1 [hat_sq][C], b1 [hat_sq], W2 [C][hat_sq], b2 [C]; innfer_net_set_chan_attn), weighted by hat_scale (conv_scale; innfer_net_set_conv_scale); per
    // residual group one OCAB behind its HABs.  sw_ln and sw_relb hold their entries in forward order: per group (norm1, norm2) / the [nH][256][256] table of every HAB, then
    // (norm1, norm2) / the [nH][256][576] table of the OCAB; sw_relb_kw: the key window of each table (16 | 24).
    int hat_cc = 0, hat_sq = 0;
    float hat_scale = 0.01f;
    std::vector<float*> hat_ca;
    std::vector<int> sw_relb_kw;
    // Swin2SR (kind 7; innfer_swin2sr_create) on SwinIR's fields, slots and workspace: cosine attention (sw_tau[blk]: nH floats, innfer_net_set_attn_scale) and the
    // LayerNorm BEHIND each branch (t = t + norm(branch)); sw_relb holds 16 sigmoid(cpb_mlp(coords)) gathered into the same dense [nH][64][64] table
    std::vector<float*> sw_tau;
    // DAT (kind 8; innfer_dat_create) on SwinIR's fields on the UNPADDED grid: split [dat_s0, dat_s1], per block whether its windows are those of the rolled frame
    // (dat_shift), the feed-forward's half padded to dat_h1p (sw_hp = 2 dat_h1p: x1's block, then x2's), and per block one device array (innfer_net_set_dat_block, the
    // order documented in the header) with the offsets below; sw_relb holds the [nH][T][T] table of the even blocks only
    int dat_s0 = 8, dat_s1 = 32, dat_h1p = 0;
    std::vector<int> dat_shift, dat_aca;         // per block (counted through the groups): shifted windows; 1 = the channel form (odd index INSIDE its group)
    std::vector<float*> dat_blk;
    std::vector<float> dat_sib2;                 // the last bias of spatial_interaction per block (a kernel argument)
    // DRCT (kind 9; innfer_drct_create) on SwinIR's fields on the grid padded to 16: dr_r dense groups of five Swin blocks; per block (counted through the groups) its head
    // count and MLP hidden size; sw_ln_w: the floats of gamma (and of beta) of every LayerNorm, in SLAB order (the dense slab's hole and pads included)
    int dr_r = 0;
    std::vector<int> dr_nh, dr_hid, sw_ln_w;
    bool span_norm = false;     // SPAN(norm=True): conv_1 reads (x - mean) * img_range through FirstConvLaunch.in_map (convs[0].d_map: alpha[in_nc] then shift[in_nc])
    int in_nc = 3, out_nc = 3, nf = 64, nb = 23, gc = 32, scale = 4, n_up = 2;
    int final_act = 0;           // `finalact` of the reference constructors: activation after the last conv (ConvLaunch.act codes)
    int band_rows = 0;
    int nr = 3;                  // dense blocks per RRDB (RRDBNet_arch.py:73-88)
    int trunk_act = 1;           // `act_type` of the constructors as a ConvLaunch.act code: 1 LeakyReLU(0.2), 2 ReLU
    bool ps_up = false;          // RRDBNet(upsample_mode='pixelshuffle'): conv nf -> 4 nf, PixelShuffle(2), act instead of Upsample, conv, act
    float res_scale = 1.f;       // SRResNet: x + res * res_scale (SRResNet_arch.py:88-91)
    int outm = 0;                // `outm` of RRDBNet / SRResNet.forward (RRDBNet_arch.py:50-62): 0 none, 1 scaltanh, 2 tanh, 3 sigmoid, 4 clamp
    int u8_normalize = 0, u8_round16 = 1;   // innfer_net_forward with INNFER_U8 images: normalize / denormalize flags of np2tensor / tensor2np, fp16 mode
    int up_phases = 1;           // upconv_block convs as four 2x2-tap phases on the LR grid (innfer_net_set_upconv_phases)
    int fused_tail = 1;          // HR_conv0 -> conv_last as one kernel where the shapes allow it (innfer_net_set_fused_tail)
    int hr_chain = 1;            // the LAST upconv_block -> HR_conv0 -> conv_last as one kernel chained through LDS (hr_chain.hip; innfer_net_set_hr_chain): the 64-channel HR tensor is never written
    int consumer_grid = 1;       // the 64-output 3x3 slab convs of the RRDBNet trunk on the 2 x 4 consumer grid (innfer_net_set_consumer_grid; conv3x3_pc GRID2); 0: the 8 x 1 form
    int res_lds = 1;             // the dense block's x5 * 0.2 + x with x taken from the conv's own staged LDS tiles (innfer_net_set_residual_lds; conv3x3_pc RLDS): 1 = where the RRDB's residual follows, 2 = every block
    bool plus = false;           // ESRGAN+ residual paths (RRDBNet_arch.py:155-160)
    int unshuffle = 1;           // innfer_rrdbnet_create_ex2: pixel_unshuffle(r) in front of the first conv (BasicSR RRDBNet scale 2 / 1), folded into that conv (conv_first_unshuffle.hip);
                                 // the forward's H x W is the image, every layer runs on the LR grid ceil(H / r) x ceil(W / r)
    int fp32 = 0;                // innfer_net_set_precision: 1 = fp32-accurate forward on split operands (conv3x3.hip SPLIT), the reference's -no_fp16 mode (run.py:345,421-422)
    std::vector<ConvSlot> convs;
};

static int n_upscale(int scale) {
    if (scale == 3) return 1;             // one Upsample(scale_factor=3) stage (RRDBNet_arch.py:33-36)
    int n = 0;
    while ((1 << n) < scale) ++n;
    return n;
}

static void add_conv(innfer_net* net, const std::string& key, int K, int C, bool first = false, int ksize = 3) {
    ConvSlot s;
    s.key = key; s.K = K; s.C = C; s.first = first; s.ksize = ksize;
    net->convs.push_back(s);
}

extern "C" int innfer_version(void) { return INNFER_ABI_VERSION; }
extern "C" const char* innfer_last_error(void) { return g_err.c_str(); }

extern "C" int innfer_rrdbnet_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                                     int gc, int scale, int plus) {
    return innfer_rrdbnet_create_ex(out, in_nc, out_nc, nf, nb, gc, scale, plus, 3, 1, 0);
}

extern "C" int innfer_rrdbnet_create_ex(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                                        int gc, int scale, int plus, int nr, int act, int pixelshuffle_up) {
    return innfer_rrdbnet_create_ex2(out, in_nc, out_nc, nf, nb, gc, scale, plus, nr, act, pixelshuffle_up, 1);
}

extern "C" int innfer_rrdbnet_create_ex2(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                                         int gc, int scale, int plus, int nr, int act, int pixelshuffle_up, int unshuffle) {
    if (!out) return set_error(INNFER_ERR_INVALID, "rrdbnet_create: null out");
    if (nr < 1 || nr > 64 || (act != 1 && act != 2))
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: nr=%d act=%d (built: nr >= 1; act 1 LeakyReLU(0.2), 2 ReLU)", nr, act);
    if (pixelshuffle_up && scale == 3 && nf != 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: PixelShuffle(3) is built for nf=64 (nf %d: 9 nf is not a multiple of 64)", nf);
    if (scale != 1 && scale != 2 && scale != 3 && scale != 4 && scale != 8 && scale != 16)
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: scale %d (built: 1, 2, 3, 4, 8, 16)", scale);
    if (nf % 32 || gc % 32 || nf <= 0 || gc <= 0 || nf > 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: nf=%d gc=%d (need nf in {32,64}, gc %% 32 == 0)", nf, gc);
    if (in_nc < 1 || in_nc > 8 || out_nc < 1 || out_nc > 16 || nb < 1)
        return set_error(INNFER_ERR_INVALID, "rrdbnet_create: in_nc=%d out_nc=%d nb=%d", in_nc, out_nc, nb);
    if (unshuffle != 1 && unshuffle != 2 && unshuffle != 4)
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: unshuffle %d (built: 1, 2, 4)", unshuffle);
    if (unshuffle > 1 && in_nc != 3)
        return set_error(INNFER_ERR_UNSUPPORTED, "rrdbnet_create: unshuffle %d with in_nc=%d (the folded pixel_unshuffle is built for in_nc 3: 12 or 48 channels into the first conv)", unshuffle, in_nc);
    innfer_net* net = new innfer_net();
    net->unshuffle = unshuffle;
    net->kind = 0; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = nf; net->nb = nb;
    net->gc = gc; net->scale = scale; net->n_up = n_upscale(scale); net->plus = plus != 0;
    net->nr = nr; net->trunk_act = act; net->ps_up = pixelshuffle_up != 0;
    add_conv(net, "model.0", nf, in_nc * unshuffle * unshuffle, true);
    for (int b = 0; b < nb; ++b)
        for (int r = 1; r <= nr; ++r) {
            char rdb[96];        // nr == 3: attributes RDB1..RDB3, else nn.Sequential `RDBs` (RRDBNet_arch.py:73-88)
            if (nr == 3) snprintf(rdb, sizeof rdb, "model.1.sub.%d.RDB%d", b, r);
            else snprintf(rdb, sizeof rdb, "model.1.sub.%d.RDBs.%d", b, r - 1);
            if (plus)            // conv1x1(nf -> gc, no bias), added to x2 (RRDBNet_arch.py:131,155-156)
                add_conv(net, std::string(rdb) + ".conv1x1", gc, nf, false, 1);
            for (int i = 1; i <= 5; ++i)
                add_conv(net, std::string(rdb) + ".conv" + std::to_string(i) + ".0", i < 5 ? gc : nf, nf + (i - 1) * gc);
        }
    add_conv(net, "model.1.sub." + std::to_string(nb), nf, nf);
    net->convs.back().map_ok = true;             // LR_conv under mode 'NAC' with a norm layer (RRDBNet_arch.py:29; block.py:246-254)
    int idx = 2;
    for (int u = 0; u < net->n_up; ++u) {        // upconv_block: Upsample, conv, act -- pixelshuffle_block: conv, PixelShuffle, act (block.py:333-361)
        if (net->ps_up) { add_conv(net, "model." + std::to_string(idx), nf * (scale == 3 ? 9 : 4), nf); net->convs.back().ps2 = scale != 3 && nf == 64; }
        else { add_conv(net, "model." + std::to_string(idx + 1), nf, nf); net->convs.back().up2x = scale != 3; }
        idx += 3;
    }
    add_conv(net, "model." + std::to_string(idx), nf, nf);
    add_conv(net, "model." + std::to_string(idx + 2), out_nc, nf);
    *out = net;
    return INNFER_OK;
}

extern "C" int innfer_srresnet_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb, int scale) {
    return innfer_srresnet_create_ex(out, in_nc, out_nc, nf, nb, scale, 2, 1.0f, 0);
}

extern "C" int innfer_srresnet_create_ex(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb, int scale, int act, float res_scale, int upconv_up) {
    if (!out) return set_error(INNFER_ERR_INVALID, "srresnet_create: null out");
    if (scale != 1 && scale != 2 && scale != 3 && scale != 4 && scale != 8)
        return set_error(INNFER_ERR_UNSUPPORTED, "srresnet_create: scale %d (built: 1, 2, 3, 4, 8)", scale);
    if (nf != 64 && nf != 32) return set_error(INNFER_ERR_UNSUPPORTED, "srresnet_create: nf=%d", nf);
    if (scale == 3 && nf != 64 && !upconv_up) return set_error(INNFER_ERR_UNSUPPORTED, "srresnet_create: PixelShuffle(3) is built for nf=64 (9 nf must be a multiple of 64)");
    if (act != 1 && act != 2) return set_error(INNFER_ERR_UNSUPPORTED, "srresnet_create: act %d (1 LeakyReLU(0.2), 2 ReLU)", act);
    if (in_nc < 1 || in_nc > 8 || out_nc < 1 || out_nc > 16 || nb < 1)
        return set_error(INNFER_ERR_INVALID, "srresnet_create: in_nc=%d out_nc=%d nb=%d", in_nc, out_nc, nb);
    innfer_net* net = new innfer_net();
    net->kind = 1; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = nf; net->nb = nb;
    net->gc = 0; net->scale = scale; net->n_up = n_upscale(scale);
    net->trunk_act = act; net->res_scale = res_scale; net->ps_up = !upconv_up;
    add_conv(net, "model.0", nf, in_nc, true);
    for (int b = 0; b < nb; ++b) {
        add_conv(net, "model.1.sub." + std::to_string(b) + ".res.0", nf, nf);
        net->convs.back().map_ok = true;
        add_conv(net, "model.1.sub." + std::to_string(b) + ".res.2", nf, nf);
    }
    add_conv(net, "model.1.sub." + std::to_string(nb), nf, nf);
    net->convs.back().map_ok = true;
    int idx = 2;
    for (int u = 0; u < net->n_up; ++u) {        // pixelshuffle_block: conv, PixelShuffle, act -- upconv_block: Upsample, conv, act (block.py:333-361)
        if (net->ps_up) { add_conv(net, "model." + std::to_string(idx), nf * (scale == 3 ? 9 : 4), nf); net->convs.back().ps2 = scale != 3 && nf == 64; }
        else { add_conv(net, "model." + std::to_string(idx + 1), nf, nf); net->convs.back().up2x = scale != 3; }
        idx += 3;
    }
    add_conv(net, "model." + std::to_string(idx), nf, nf);
    add_conv(net, "model." + std::to_string(idx + 2), out_nc, nf);
    *out = net;
    return INNFER_OK;
}

// BasicSR's SRVGGNetCompact (realesr-animevideov3, realesr-general-x4v3, the community "compact" models): `body`, a chain of 3x3 convs on the LR grid -- body.0
// (in_nc -> nf) and num_conv convs nf -> nf, each followed by its activation (PReLU(nf) / ReLU / LeakyReLU(0.1): per-channel slopes, innfer_net_set_conv_slope),
// then body.<2 num_conv + 2> (nf -> out_nc scale^2, no activation); out = PixelShuffle(scale)(body(x)) + nearest_upsample(x, scale).  fp16 engine only.
extern "C" int innfer_compact_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int num_conv, int scale) {
    if (!out) return set_error(INNFER_ERR_INVALID, "compact_create: null out");
    if (nf != 32 && nf != 64) return set_error(INNFER_ERR_UNSUPPORTED, "compact_create: nf=%d (built: 32, 64; fewer features are zero-padded by the caller)", nf);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc)
        return set_error(INNFER_ERR_UNSUPPORTED, "compact_create: in_nc=%d out_nc=%d (built: in_nc == out_nc in 1..4 -- the network adds its upsampled input to its result)", in_nc, out_nc);
    if (num_conv < 0 || num_conv > 4096) return set_error(INNFER_ERR_UNSUPPORTED, "compact_create: num_conv=%d", num_conv);
    if (scale < 1 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "compact_create: scale %d (built: 1, 2, 3, 4)", scale);
    innfer_net* net = new innfer_net();
    net->kind = 2; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = nf; net->nb = num_conv;
    net->gc = 0; net->scale = scale; net->n_up = 0;
    add_conv(net, "body.0", nf, in_nc, true);
    net->convs.back().slope_ok = true;
    for (int i = 1; i <= num_conv; ++i) {
        add_conv(net, "body." + std::to_string(2 * i), nf, nf);
        net->convs.back().slope_ok = true;
    }
    add_conv(net, "body." + std::to_string(2 * num_conv + 2), out_nc * scale * scale, nf);
    net->convs.back().Kp = out_nc * scale * scale <= 32 ? 32 : 64;
    *out = net;
    return INNFER_OK;
}

// SPAN (Swift Parameter-free Attention Network; the reference has no such architecture -- include/innfer_amd.h carries the definition): 3x3 convs on the LR grid with
// SiLU (act 9) and gate (act 10) epilogues.  The convs are the COLLAPSED Conv3XC (one 3x3 conv each, folded by the caller), conv_cat (1x1 over the 4 nf-channel concat) and
// upsampler.0 (nf -> out_nc scale^2, PixelShuffle in shuffle_add_launch without a base).  fp16 engine only.
extern "C" int innfer_span_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int scale, int norm, float img_range, const float* mean) {
    if (!out) return set_error(INNFER_ERR_INVALID, "span_create: null out");
    if (nf != 32 && nf != 64) return set_error(INNFER_ERR_UNSUPPORTED, "span_create: nf=%d (built: 32, 64; fewer features are zero-padded by the caller)", nf);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc)
        return set_error(INNFER_ERR_UNSUPPORTED, "span_create: in_nc=%d out_nc=%d (built: in_nc == out_nc in 1..4)", in_nc, out_nc);
    if (scale < 1 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "span_create: scale %d (built: 1, 2, 3, 4)", scale);
    if (norm && !mean) return set_error(INNFER_ERR_INVALID, "span_create: norm needs the %d channel means", in_nc);
    innfer_net* net = new innfer_net();
    net->kind = 3; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = nf; net->nb = 6;
    net->gc = 0; net->scale = scale; net->n_up = 0;
    net->span_norm = norm != 0;
    add_conv(net, "conv_1", nf, in_nc, true);
    for (int b = 1; b <= 6; ++b)
        for (int j = 1; j <= 3; ++j) add_conv(net, "block_" + std::to_string(b) + ".c" + std::to_string(j) + "_r", nf, nf);
    add_conv(net, "conv_2", nf, nf);
    add_conv(net, "conv_cat", nf, 4 * nf, false, 1);
    add_conv(net, "upsampler.0", out_nc * scale * scale, nf);
    net->convs.back().Kp = out_nc * scale * scale <= 32 ? 32 : 64;
    if (norm) {                  // (x - mean[c]) * img_range = img_range * x - mean[c] * img_range, x = the fp16 tensor value / np2tensor of the uint8 image
        float h[8];
        for (int c = 0; c < in_nc; ++c) { h[c] = img_range; h[in_nc + c] = -mean[c] * img_range; }
        ConvSlot& c0 = net->convs[0];
        if (hipMalloc((void**)&c0.d_map, 2 * in_nc * sizeof(float)) != hipSuccess || hipMemcpy(c0.d_map, h, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            innfer_net_destroy(net);
            return set_error(INNFER_ERR_NOMEM, "span_create: no device memory for the input map");
        }
    }
    *out = net;
    return INNFER_OK;
}

// RealPLKSR (the reference has no such architecture -- include/innfer_amd.h carries the definition): per block DCCM (3x3 64 -> 128 with Mish as two 64-output launches
// of act 11, 3x3 128 -> 64), the partial large-kernel conv (plk_conv.hip), the EA gate (3x3 64 -> 64, act 5 on its own input), refine (1x1) and GroupNorm + skip
// (group_norm.hip); the tail is SRVGGNetCompact's.  fp16 engine only.
extern "C" int innfer_plksr_create(innfer_net_t* out, int in_nc, int out_nc, int dim, int n_blocks, int scale, int kernel_size, int use_ea, int norm_groups) {
    if (!out) return set_error(INNFER_ERR_INVALID, "plksr_create: null out");
    if (dim != 64) return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: dim=%d (built: 64, with the large kernel on its first 16 channels)", dim);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc)
        return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: in_nc=%d out_nc=%d (built: in_nc == out_nc in 1..4 -- the network adds its repeated input to its result)", in_nc, out_nc);
    if (n_blocks < 1 || n_blocks > 4096) return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: n_blocks=%d", n_blocks);
    if (scale < 1 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: scale %d (built: 1, 2, 3, 4)", scale);
    if (kernel_size < 3 || kernel_size > 17 || !(kernel_size & 1)) return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: kernel_size %d (built: odd, 3 .. 17)", kernel_size);
    if (norm_groups != 1 && norm_groups != 2 && norm_groups != 4 && norm_groups != 8)
        return set_error(INNFER_ERR_UNSUPPORTED, "plksr_create: norm_groups %d (built: 1, 2, 4, 8)", norm_groups);
    innfer_net* net = new innfer_net();
    net->kind = 4; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = dim; net->nb = n_blocks;
    net->gc = 0; net->scale = scale; net->n_up = 0;
    net->plk_k = kernel_size; net->plk_ea = use_ea != 0; net->plk_groups = norm_groups;
    add_conv(net, "feats.0", dim, in_nc, true);
    for (int b = 1; b <= n_blocks; ++b) {
        const std::string p = "feats." + std::to_string(b) + ".";
        add_conv(net, p + "channel_mixer.0a", dim, dim);              // output channels 0 .. 63 and 64 .. 127 of channel_mixer.0: one 64-output launch each
        add_conv(net, p + "channel_mixer.0b", dim, dim);
        add_conv(net, p + "channel_mixer.2", dim, 2 * dim);
        add_conv(net, p + "lk.conv", 16, 16, false, kernel_size);
        net->convs.back().plk = true;
        if (use_ea) { add_conv(net, p + "attn.f.0", dim, dim); net->convs.back().lane_rows = true; }
        add_conv(net, p + "refine", dim, dim, false, 1);
        net->convs.back().gn_ok = true;
    }
    add_conv(net, "feats." + std::to_string(n_blocks + 2), out_nc * scale * scale, dim);
    net->convs.back().Kp = out_nc * scale * scale <= 32 ? 32 : 64;
    *out = net;
    return INNFER_OK;
}

// SwinIR (Liang et al. 2021; the reference has no such architecture -- include/innfer_amd.h carries the definition) on 8 x 8 windows.  Every Linear and every conv from or
// to the C_pad-channel token slab is a chain of 64-output launches, one ConvSlot each (key `<state-dict key>#<p>`: output channels 64 p .. 64 p + 63 of the RE-LAID-OUT
// weight the caller passes: input channels padded with zeros, qkv rows in the head-padded order, proj columns likewise).  fp16 engine only.
static void swin_add_sliced(innfer_net* net, const std::string& key, int Kp, int C, int ksize, float mult = 1.f) {
    for (int p = 0; p < Kp / 64; ++p) {
        add_conv(net, key + "#" + std::to_string(p), 64, C, false, ksize);
        net->convs.back().mult = mult;
    }
}
static void swin_add_resi(innfer_net* net, const std::string& key) {          // resi_connection: '1conv' a 3x3 conv, '3conv' 3x3 C -> C / 4, 1x1, 3x3 C / 4 -> C with LeakyReLU(0.2) between
    if (!net->sw_conv3) { swin_add_sliced(net, key, net->sw_cp, net->sw_cp, 3); return; }
    swin_add_sliced(net, key + ".0", net->sw_c4p, net->sw_cp, 3);
    swin_add_sliced(net, key + ".2", net->sw_c4p, net->sw_c4p, 1);
    swin_add_sliced(net, key + ".4", net->sw_cp, net->sw_c4p, 3);
}
static int swin_create(int kind, innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int upsampler,
                       int scale, int conv3, const float* h_mean) {
    if (!out || !depths) return set_error(INNFER_ERR_INVALID, "swinir_create: null argument");
    if (embed_dim < 1 || embed_dim > 256 || num_heads < 1 || num_heads > 8 || embed_dim % num_heads || embed_dim / num_heads > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: embed_dim=%d num_heads=%d (built: embed_dim <= 256, <= 8 heads of <= 32 channels, embed_dim %% num_heads == 0)", embed_dim, num_heads);
    if (mlp_hidden < 1 || mlp_hidden > 1024) return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: an MLP of %d hidden channels (built: <= 1024)", mlp_hidden);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc)
        return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: in_chans=%d, %d output channels (built: equal, 1..4)", in_nc, out_nc);
    if (n_layers < 1 || n_layers > 64) return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: %d residual groups", n_layers);
    for (int i = 0; i < n_layers; ++i)
        if (depths[i] < 1 || depths[i] > 64) return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: depth %d of residual group %d", depths[i], i);
    if (upsampler < 0 || upsampler > 2) return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: upsampler %d (0 pixelshuffle, 1 pixelshuffledirect, 2 nearest+conv)", upsampler);
    if ((upsampler == 2 && scale != 2 && scale != 4) || (upsampler != 2 && (scale < 2 || scale > 4)))
        return set_error(INNFER_ERR_UNSUPPORTED, "swinir_create: scale %d (built: 2, 3, 4 with pixelshuffle / pixelshuffledirect, 2 and 4 with nearest+conv)", scale);
    innfer_net* net = new innfer_net();
    net->kind = kind; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = 64; net->nb = 0; net->gc = 0; net->scale = scale; net->n_up = 0;
    net->sw_c = embed_dim; net->sw_cp = (embed_dim + 63) / 64 * 64; net->sw_nh = num_heads; net->sw_d = embed_dim / num_heads;
    net->sw_hid = mlp_hidden; net->sw_hp = (mlp_hidden + 63) / 64 * 64; net->sw_tail = upsampler; net->sw_conv3 = conv3 != 0;
    net->sw_c4p = (embed_dim / 4 + 63) / 64 * 64;
    net->sw_depths.assign(depths, depths + n_layers);
    const int cp = net->sw_cp;
    for (int p = 0; p < cp / 64; ++p) add_conv(net, "conv_first#" + std::to_string(p), 64, in_nc, true);
    for (int i = 0; i < n_layers; ++i) {
        for (int j = 0; j < depths[i]; ++j) {
            const std::string b = "layers." + std::to_string(i) + ".residual_group.blocks." + std::to_string(j) + ".";
            swin_add_sliced(net, b + "attn.qkv", (3 * num_heads + 1) / 2 * 64, cp, 1);
            swin_add_sliced(net, b + "attn.proj", cp, 32 * num_heads, 1);
            swin_add_sliced(net, b + "mlp.fc1", net->sw_hp, cp, 1);
            swin_add_sliced(net, b + "mlp.fc2", cp, net->sw_hp, 1);
            net->nb++;
        }
        swin_add_resi(net, "layers." + std::to_string(i) + ".conv");
    }
    swin_add_resi(net, "conv_after_body");
    const float s2 = (float)(scale * scale);
    if (upsampler == 1) {
        add_conv(net, "upsample.0", out_nc * scale * scale, cp);
        net->convs.back().Kp = out_nc * scale * scale <= 32 ? 32 : 64;
    } else {
        add_conv(net, "conv_before_upsample.0", 64, cp);
        net->convs.back().slope_ok = true;
        if (upsampler == 0) {
            if (scale == 3) add_conv(net, "upsample.0", 576, 64);
            else {
                add_conv(net, "upsample.0", 256, 64); net->convs.back().ps2 = true;
                if (scale == 4) { add_conv(net, "upsample.2", 256, 64); net->convs.back().ps2 = true; net->convs.back().mult = 4.f; }
            }
        } else {
            add_conv(net, "conv_up1", 64, 64); net->convs.back().mult = 4.f;
            if (scale == 4) { add_conv(net, "conv_up2", 64, 64); net->convs.back().mult = 16.f; }
            add_conv(net, "conv_hr", 64, 64); net->convs.back().mult = s2;
        }
        add_conv(net, "conv_last", out_nc, 64); net->convs.back().mult = s2;
    }
    net->sw_ln.assign(2 + 2 * (size_t)net->nb, nullptr);
    net->sw_relb.assign((size_t)net->nb, nullptr);
    if (kind == 7) net->sw_tau.assign((size_t)net->nb, nullptr);
    int rc = INNFER_OK;
    {   // x - mean in front of conv_first (img_range 1): the input map of every slice of the first conv, held by slice 0; nn.LeakyReLU() (slope 0.01) behind conv_before_upsample
        float h[8];
        for (int c = 0; c < in_nc; ++c) { h[c] = 1.f; h[in_nc + c] = h_mean ? -h_mean[c] : 0.f; }
        ConvSlot& c0 = net->convs[0];
        if (hipMalloc((void**)&c0.d_map, 2 * in_nc * sizeof(float)) != hipSuccess || hipMemcpy(c0.d_map, h, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_error(INNFER_ERR_NOMEM, "swinir_create: no device memory for the input map");
        for (size_t i = 0; i < net->convs.size() && rc == INNFER_OK; ++i)
            if (net->convs[i].slope_ok) {
                const std::vector<float> sl(64, 0.01f);
                rc = innfer_net_set_conv_slope(net, (int)i, sl.data());
            }
    }
    if (rc != INNFER_OK) { (void)hipGetLastError(); innfer_net_destroy(net); return rc; }
    *out = net;
    return INNFER_OK;
}

extern "C" int innfer_swinir_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int upsampler,
                                    int scale, int conv3, const float* h_mean) {
    return swin_create(5, out, in_nc, out_nc, embed_dim, depths, n_layers, num_heads, mlp_hidden, upsampler, scale, conv3, h_mean);
}
// Swin2SR (Conde et al. 2022; include/innfer_amd.h carries the definition): SwinIR's skeleton, conv slots, LayerNorm numbering, tails and workspace; the block is
// t = t + norm1(proj(attn(t))), t = t + norm2(fc2(GELU(fc1(t)))) with the cosine attention.  Arguments, limits and refusals are innfer_swinir_create's.
extern "C" int innfer_swin2sr_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int upsampler,
                                     int scale, int conv3, const float* h_mean) {
    return swin_create(7, out, in_nc, out_nc, embed_dim, depths, n_layers, num_heads, mlp_hidden, upsampler, scale, conv3, h_mean);
}

// DRCT's widths: gx = ceil(C / 32) groups of x; block k = 0 .. 4 of a dense group reads ng[k] = gx + k groups (cpk[k] = 32 ng[k] channels: what a matrix product reads),
// lp[k] = cpk[k] rounded up to 64 (what a LayerNorm covers and a chain of 64-output launches writes); per block b the head groups G = ceil(d / 32), nH G groups of q
struct DrctDims { int gx, ng[5], cpk[5], lp[5], dense_groups, max_sq, max_hg, max_hp; };
static int drct_head_groups(const innfer_net* net, size_t b) { const int d = (net->sw_c + 32 * (int)(b % 5)) / net->dr_nh[b]; return net->dr_nh[b] * ((d + 31) / 32); }
static DrctDims drct_dims(const innfer_net* net) {
    DrctDims d{};
    d.gx = (net->sw_c + 31) / 32;
    for (int k = 0; k < 5; ++k) { d.ng[k] = d.gx + k; d.cpk[k] = 32 * d.ng[k]; d.lp[k] = (d.cpk[k] + 63) / 64 * 64; }
    d.dense_groups = (d.gx + 5 + 1) / 2 * 2;
    for (size_t b = 0; b < net->dr_nh.size(); ++b) {
        const int hg = drct_head_groups(net, b);
        d.max_hg = std::max(d.max_hg, hg);
        d.max_sq = std::max(d.max_sq, (3 * hg + 1) / 2);
        d.max_hp = std::max(d.max_hp, (net->dr_hid[b] + 63) / 64 * 64);
    }
    return d;
}
// DRCT (Hsu et al. 2024; include/innfer_amd.h carries the definition): n_groups dense groups of five Swin blocks on 16 x 16 windows.  Block k = 0 .. 4 of a group works on
// dim_k = C + 32 k channels with h_heads[5 g + k] heads and an MLP of h_hidden[5 g + k] channels.  torch.cat is a slab layout: x in its own ceil(C / 32) groups, x_k in one
// group each behind them; the caller passes every weight with its input columns in that order (zero columns at the hole [C, 32 ceil(C / 32)) and the pads).  Conv slots
// `<state-dict key>#<p>` in forward order: conv_first; per block attn.qkv (ceil(3 nH G / 2) slices of [64, 32 ng]), attn.proj (lp / 64 slices of [64, 32 nH G]), mlp.fc1,
// mlp.fc2, adjust (one slice for k < 4: 32 real rows, 32 zero rows that clear the next group; C_pad / 64 slices for k = 4); conv_after_body; the pixelshuffle tail.
// Launches of a forward, with S1 = C_pad / 64, per block S = lp_k / 64, SQ = ceil(3 nH G / 2), SH = hidden_pad / 64, A = 1 (k < 4) | S1 (k = 4), T = 2 + log2(scale) (4 for 3):
//   2 S1 + 2 + sum over blocks (3 + SQ + 2 S + SH + A) + T + 2 [H x W is not Hp x Wp]
extern "C" int innfer_drct_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, int n_groups, const int* h_heads, const int* h_hidden, int scale, const float* h_mean) {
    if (!out || !h_heads || !h_hidden) return set_error(INNFER_ERR_INVALID, "drct_create: null argument");
    if (embed_dim < 1 || embed_dim > 256) return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: embed_dim=%d (built: 1 .. 256)", embed_dim);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc) return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: in_chans=%d, %d output channels (built: equal, 1..4)", in_nc, out_nc);
    if (n_groups < 1 || n_groups > 64) return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: %d dense groups", n_groups);
    if (scale < 2 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: scale %d (built: 2, 3, 4 -- the pixelshuffle tail)", scale);
    for (int b = 0; b < 5 * n_groups; ++b) {
        const int dim = embed_dim + 32 * (b % 5), nh = h_heads[b];
        if (nh < 1 || nh > 8 || dim % nh || dim / nh > 128)
            return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: block %d has %d heads on %d channels (built: <= 8 heads of <= 128 channels, dim %% heads == 0)", b, nh, dim);
        if (h_hidden[b] < 1 || h_hidden[b] > 1024) return set_error(INNFER_ERR_UNSUPPORTED, "drct_create: an MLP of %d hidden channels in block %d (built: <= 1024)", h_hidden[b], b);
    }
    innfer_net* net = new innfer_net();
    net->kind = 9; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = 64; net->nb = 5 * n_groups; net->gc = 0; net->scale = scale; net->n_up = 0;
    net->sw_c = embed_dim; net->sw_cp = (embed_dim + 63) / 64 * 64; net->sw_tail = 0; net->sw_conv3 = 0;
    net->dr_r = n_groups;
    net->dr_nh.assign(h_heads, h_heads + 5 * n_groups);
    net->dr_hid.assign(h_hidden, h_hidden + 5 * n_groups);
    const DrctDims dd = drct_dims(net);
    const int cp = net->sw_cp;
    net->sw_hp = dd.max_hp;
    for (int p = 0; p < cp / 64; ++p) add_conv(net, "conv_first#" + std::to_string(p), 64, in_nc, true);
    net->sw_ln_w.push_back(cp);
    for (int i = 0; i < n_groups; ++i)
        for (int k = 0; k < 5; ++k) {
            const size_t b = (size_t)5 * i + k;
            const std::string g = "layers." + std::to_string(i) + ".", sw = g + "swin" + std::to_string(k + 1) + ".";
            const int hg = drct_head_groups(net, b), hp = (net->dr_hid[b] + 63) / 64 * 64;
            swin_add_sliced(net, sw + "attn.qkv", (3 * hg + 1) / 2 * 64, dd.cpk[k], 1);
            swin_add_sliced(net, sw + "attn.proj", dd.lp[k], 32 * hg, 1);
            swin_add_sliced(net, sw + "mlp.fc1", hp, dd.cpk[k], 1);
            swin_add_sliced(net, sw + "mlp.fc2", dd.lp[k], hp, 1);
            swin_add_sliced(net, g + "adjust" + std::to_string(k + 1), k < 4 ? 64 : cp, dd.cpk[k], 1);
            net->sw_ln_w.push_back(dd.lp[k]); net->sw_ln_w.push_back(dd.lp[k]);
        }
    net->sw_ln_w.push_back(cp);
    swin_add_sliced(net, "conv_after_body", cp, cp, 3);
    add_conv(net, "conv_before_upsample.0", 64, cp);
    net->convs.back().slope_ok = true;
    const float s2 = (float)(scale * scale);
    if (scale == 3) add_conv(net, "upsample.0", 576, 64);
    else {
        add_conv(net, "upsample.0", 256, 64); net->convs.back().ps2 = true;
        if (scale == 4) { add_conv(net, "upsample.2", 256, 64); net->convs.back().ps2 = true; net->convs.back().mult = 4.f; }
    }
    add_conv(net, "conv_last", out_nc, 64); net->convs.back().mult = s2;
    net->sw_ln.assign(net->sw_ln_w.size(), nullptr);
    net->sw_relb.assign((size_t)net->nb, nullptr);
    int rc = INNFER_OK;
    {   // x - mean in front of conv_first and nn.LeakyReLU() behind conv_before_upsample, as swin_create
        float h[8];
        for (int c = 0; c < in_nc; ++c) { h[c] = 1.f; h[in_nc + c] = h_mean ? -h_mean[c] : 0.f; }
        ConvSlot& c0 = net->convs[0];
        if (hipMalloc((void**)&c0.d_map, 2 * in_nc * sizeof(float)) != hipSuccess || hipMemcpy(c0.d_map, h, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_error(INNFER_ERR_NOMEM, "drct_create: no device memory for the input map");
        for (size_t i = 0; i < net->convs.size() && rc == INNFER_OK; ++i)
            if (net->convs[i].slope_ok) {
                const std::vector<float> sl(64, 0.01f);
                rc = innfer_net_set_conv_slope(net, (int)i, sl.data());
            }
    }
    if (rc != INNFER_OK) { (void)hipGetLastError(); innfer_net_destroy(net); return rc; }
    *out = net;
    return INNFER_OK;
}

// gamma / beta (C host floats each) of LayerNorm `idx` of a SwinIR: 0 patch_embed.norm, 1 + 2 b / 2 + 2 b norm1 / norm2 of block b (blocks counted through the residual
// groups), the last one norm.  Load time, synchronous.
extern "C" int innfer_net_set_layer_norm(innfer_net_t net, int idx, const float* h_gamma, const float* h_beta) {
    if (!net || !h_gamma || !h_beta) return set_error(INNFER_ERR_INVALID, "set_layer_norm: null argument");
    if (net->kind != 5 && net->kind != 6 && net->kind != 7 && net->kind != 8 && net->kind != 9) return set_error(INNFER_ERR_UNSUPPORTED, "set_layer_norm: the network has no LayerNorm (built: SwinIR, HAT, Swin2SR, DAT, DRCT)");
    if (idx < 0 || idx >= (int)net->sw_ln.size()) return set_error(INNFER_ERR_INVALID, "set_layer_norm: index %d of %zu", idx, net->sw_ln.size());
    if (net->kind == 9) {        // DRCT: sw_ln_w[idx] floats each, already in the slab order of the tensor the norm reads (zeros at the hole and the pads)
        const size_t wdt = (size_t)net->sw_ln_w[idx];
        std::vector<float> h(2 * wdt);
        std::copy(h_gamma, h_gamma + wdt, h.begin());
        std::copy(h_beta, h_beta + wdt, h.begin() + wdt);
        if (!net->sw_ln[idx]) INNFER_HIP(hipMalloc((void**)&net->sw_ln[idx], h.size() * sizeof(float)));
        INNFER_HIP(hipMemcpy(net->sw_ln[idx], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        return INNFER_OK;
    }
    std::vector<float> h(2 * (size_t)net->sw_cp, 0.f);
    for (int c = 0; c < net->sw_c; ++c) { h[c] = h_gamma[c]; h[net->sw_cp + c] = h_beta[c]; }
    if (!net->sw_ln[idx]) INNFER_HIP(hipMalloc((void**)&net->sw_ln[idx], h.size() * sizeof(float)));
    INNFER_HIP(hipMemcpy(net->sw_ln[idx], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return INNFER_OK;
}

// The relative position bias of block `blk` of a SwinIR as the dense table the attention reads: [num_heads][64 query][64 key] host floats.  Load time, synchronous.
extern "C" int innfer_net_set_attn_bias(innfer_net_t net, int blk, const float* h_bias) {
    if (!net || !h_bias) return set_error(INNFER_ERR_INVALID, "set_attn_bias: null argument");
    if (net->kind != 5 && net->kind != 6 && net->kind != 7 && net->kind != 8 && net->kind != 9) return set_error(INNFER_ERR_UNSUPPORTED, "set_attn_bias: the network has no window attention (built: SwinIR, HAT, Swin2SR, DAT, DRCT)");
    if (blk < 0 || blk >= (int)net->sw_relb.size()) return set_error(INNFER_ERR_INVALID, "set_attn_bias: block %d of %zu", blk, net->sw_relb.size());
    // (HAT: table `blk` in forward order -- [num_heads][256][256] of a HAB, [num_heads][256][576] of a residual group's OCAB)
    // (DAT: [num_heads][T][T], T = s0 s1, of an even block; the odd blocks take none)
    const size_t dat_t = (size_t)net->dat_s0 * net->dat_s1;
    // (DRCT: [nH_blk][256][256] with the block's own head count)
    const size_t nb = net->kind == 9 ? (size_t)net->dr_nh[blk] * 65536 * sizeof(float) : (size_t)net->sw_nh * (net->kind == 6 ? 256 * (size_t)net->sw_relb_kw[blk] * net->sw_relb_kw[blk] : net->kind == 8 ? dat_t * dat_t : 4096) * sizeof(float);
    if (!net->sw_relb[blk]) INNFER_HIP(hipMalloc((void**)&net->sw_relb[blk], nb));
    INNFER_HIP(hipMemcpy(net->sw_relb[blk], h_bias, nb, hipMemcpyHostToDevice));
    return INNFER_OK;
}

// tau of block `blk` of a Swin2SR: exp(min(logit_scale, ln 100)) of every head, num_heads host floats (finite, > 0).  Load time, synchronous.
extern "C" int innfer_net_set_attn_scale(innfer_net_t net, int blk, const float* h_tau) {
    if (!net || !h_tau) return set_error(INNFER_ERR_INVALID, "set_attn_scale: null argument");
    if (net->kind != 7) return set_error(INNFER_ERR_UNSUPPORTED, "set_attn_scale: the network has no cosine attention (built: Swin2SR)");
    if (blk < 0 || blk >= (int)net->sw_tau.size()) return set_error(INNFER_ERR_INVALID, "set_attn_scale: block %d of %zu", blk, net->sw_tau.size());
    for (int h = 0; h < net->sw_nh; ++h)
        if (!(h_tau[h] > 0.f) || !std::isfinite(h_tau[h])) return set_error(INNFER_ERR_INVALID, "set_attn_scale: tau[%d] = %g of block %d (finite, > 0)", h, (double)h_tau[h], blk);
    if (!net->sw_tau[blk]) INNFER_HIP(hipMalloc((void**)&net->sw_tau[blk], (size_t)net->sw_nh * sizeof(float)));
    INNFER_HIP(hipMemcpy(net->sw_tau[blk], h_tau, (size_t)net->sw_nh * sizeof(float), hipMemcpyHostToDevice));
    return INNFER_OK;
}

// HAT (Chen et al. 2023; include/innfer_amd.h carries the definition) on SwinIR's skeleton with 16 x 16 windows: per HAB the conv block (two 3x3 convs around a GELU, channel
// attention) beside the window attention, per residual group one overlapping cross-attention block behind its HABs.  Conv slots in forward order; keys as SwinIR's.
extern "C" int innfer_hat_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int compress_ch,
                                 int squeeze_ch, int scale, const float* h_mean) {
    if (!out || !depths) return set_error(INNFER_ERR_INVALID, "hat_create: null argument");
    if (embed_dim < 1 || embed_dim > 256 || num_heads < 1 || num_heads > 8 || embed_dim % num_heads || embed_dim / num_heads > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: embed_dim=%d num_heads=%d (built: embed_dim <= 256, <= 8 heads of <= 32 channels, embed_dim %% num_heads == 0)", embed_dim, num_heads);
    if (mlp_hidden < 1 || mlp_hidden > 1024) return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: an MLP of %d hidden channels (built: <= 1024)", mlp_hidden);
    if (compress_ch < 1 || compress_ch > 64 || squeeze_ch < 1 || squeeze_ch > 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: a conv block of %d channels, a channel attention of %d (built: 1 .. 64 each)", compress_ch, squeeze_ch);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc) return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: in_chans=%d, %d output channels (built: equal, 1..4)", in_nc, out_nc);
    if (n_layers < 1 || n_layers > 64) return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: %d residual groups", n_layers);
    for (int i = 0; i < n_layers; ++i)
        if (depths[i] < 1 || depths[i] > 64) return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: depth %d of residual group %d", depths[i], i);
    if (scale < 2 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "hat_create: scale %d (built: 2, 3, 4 -- the pixelshuffle tail)", scale);
    innfer_net* net = new innfer_net();
    net->kind = 6; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = 64; net->nb = 0; net->gc = 0; net->scale = scale; net->n_up = 0;
    net->sw_c = embed_dim; net->sw_cp = (embed_dim + 63) / 64 * 64; net->sw_nh = num_heads; net->sw_d = embed_dim / num_heads;
    net->sw_hid = mlp_hidden; net->sw_hp = (mlp_hidden + 63) / 64 * 64; net->sw_tail = 0; net->sw_conv3 = 0;
    net->hat_cc = compress_ch; net->hat_sq = squeeze_ch;
    net->sw_depths.assign(depths, depths + n_layers);
    const int cp = net->sw_cp;
    for (int p = 0; p < cp / 64; ++p) add_conv(net, "conv_first#" + std::to_string(p), 64, in_nc, true);
    auto attn_mlp = [&](const std::string& b, const std::string& a) {
        swin_add_sliced(net, b + a + "qkv", (3 * num_heads + 1) / 2 * 64, cp, 1);
        swin_add_sliced(net, b + a + "proj", cp, 32 * num_heads, 1);
        swin_add_sliced(net, b + "mlp.fc1", net->sw_hp, cp, 1);
        swin_add_sliced(net, b + "mlp.fc2", cp, net->sw_hp, 1);
    };
    for (int i = 0; i < n_layers; ++i) {
        const std::string g = "layers." + std::to_string(i) + ".residual_group.";
        for (int j = 0; j < depths[i]; ++j) {
            const std::string b = g + "blocks." + std::to_string(j) + ".";
            swin_add_sliced(net, b + "conv_block.cab.0", 64, cp, 3);
            net->convs.back().lane_rows = true;          // (act 13 is an epilogue of the lane-contiguous panels only)
            swin_add_sliced(net, b + "conv_block.cab.2", cp, 64, 3);
            attn_mlp(b, "attn.");
            net->sw_relb_kw.push_back(16);
            net->nb++;
        }
        attn_mlp(g + "overlap_attn.", "");              // (overlap_attn.qkv / .proj / .mlp.fc1 / .mlp.fc2)
        net->sw_relb_kw.push_back(24);
        swin_add_sliced(net, "layers." + std::to_string(i) + ".conv", cp, cp, 3);
    }
    swin_add_sliced(net, "conv_after_body", cp, cp, 3);
    add_conv(net, "conv_before_upsample.0", 64, cp);
    net->convs.back().slope_ok = true;
    if (scale == 3) add_conv(net, "upsample.0", 576, 64);
    else {
        add_conv(net, "upsample.0", 256, 64); net->convs.back().ps2 = true;
        if (scale == 4) { add_conv(net, "upsample.2", 256, 64); net->convs.back().ps2 = true; net->convs.back().mult = 4.f; }
    }
    add_conv(net, "conv_last", out_nc, 64); net->convs.back().mult = (float)(scale * scale);
    net->sw_ln.assign(2 + 2 * ((size_t)net->nb + n_layers), nullptr);
    net->sw_relb.assign(net->sw_relb_kw.size(), nullptr);
    net->hat_ca.assign((size_t)net->nb, nullptr);
    int rc = INNFER_OK;
    {   // x - mean in front of conv_first and nn.LeakyReLU() (slope 0.01) behind conv_before_upsample, as innfer_swinir_create
        float h[8];
        for (int c = 0; c < in_nc; ++c) { h[c] = 1.f; h[in_nc + c] = h_mean ? -h_mean[c] : 0.f; }
        ConvSlot& c0 = net->convs[0];
        if (hipMalloc((void**)&c0.d_map, 2 * in_nc * sizeof(float)) != hipSuccess || hipMemcpy(c0.d_map, h, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_error(INNFER_ERR_NOMEM, "hat_create: no device memory for the input map");
        for (size_t i = 0; i < net->convs.size() && rc == INNFER_OK; ++i)
            if (net->convs[i].slope_ok) {
                const std::vector<float> sl(64, 0.01f);
                rc = innfer_net_set_conv_slope(net, (int)i, sl.data());
            }
    }
    if (rc != INNFER_OK) { (void)hipGetLastError(); innfer_net_destroy(net); return rc; }
    *out = net;
    return INNFER_OK;
}

// The channel attention of HAB `blk` of a HAT (blocks counted through the residual groups): the two 1x1 convs behind the pool as host floats, W1 [squeeze_ch][C], b1
// [squeeze_ch], W2 [C][squeeze_ch], b2 [C].  Load time, synchronous.
extern "C" int innfer_net_set_chan_attn(innfer_net_t net, int blk, const float* h_w1, const float* h_b1, const float* h_w2, const float* h_b2) {
    if (!net || !h_w1 || !h_b1 || !h_w2 || !h_b2) return set_error(INNFER_ERR_INVALID, "set_chan_attn: null argument");
    if (net->kind != 6) return set_error(INNFER_ERR_UNSUPPORTED, "set_chan_attn: the network has no channel attention (built: HAT)");
    if (blk < 0 || blk >= (int)net->hat_ca.size()) return set_error(INNFER_ERR_INVALID, "set_chan_attn: block %d of %zu", blk, net->hat_ca.size());
    const size_t C = (size_t)net->sw_c, q = (size_t)net->hat_sq;
    std::vector<float> h;
    h.insert(h.end(), h_w1, h_w1 + q * C); h.insert(h.end(), h_b1, h_b1 + q);
    h.insert(h.end(), h_w2, h_w2 + C * q); h.insert(h.end(), h_b2, h_b2 + C);
    if (!net->hat_ca[blk]) INNFER_HIP(hipMalloc((void**)&net->hat_ca[blk], h.size() * sizeof(float)));
    INNFER_HIP(hipMemcpy(net->hat_ca[blk], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return INNFER_OK;
}

// conv_scale of a HAT: the weight of the conv block beside the attention (a constructor argument of the published code, not in the state dict; 0.01 by default)
extern "C" int innfer_net_set_conv_scale(innfer_net_t net, float conv_scale) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_conv_scale: null argument");
    if (net->kind != 6) return set_error(INNFER_ERR_UNSUPPORTED, "set_conv_scale: the network has no conv block (built: HAT)");
    if (!(conv_scale == conv_scale) || std::fabs(conv_scale) > 65504.f) return set_error(INNFER_ERR_INVALID, "set_conv_scale: %g", (double)conv_scale);
    net->hat_scale = conv_scale;
    return INNFER_OK;
}

// DAT (Chen et al. 2023; include/innfer_amd.h carries the definition) on SwinIR's skeleton WITHOUT padding: blocks alternate between attention over rectangular windows
// (even b) and attention across channels (odd b); both end in the interaction mix with a depthwise conv of v; the feed-forward is gated by a depthwise conv of its
// second half.  Conv slots in forward order: conv_first; per block attn.qkv, attn.proj (input: the head-padded 32 nH channels), ffn.fc1 (rows: x1's block padded to
// dat_h1p, then x2's), ffn.fc2 (input: dat_h1p channels); per group its conv; conv_after_body; the tail.
struct DatOff { size_t dw_t, dw_b, ci_w1, ci_b1, ci_w2, ci_b2, si_w1, si_b1, si_w2, si_b2, sg_g, sg_b, sg_t, sg_cb, temp, total; };
static DatOff dat_offsets(const innfer_net* net) {
    const size_t ch = 32 * (size_t)net->sw_nh, hc = (size_t)net->sw_c / 8, hs = (size_t)net->sw_c / 16, half = (size_t)net->sw_hid / 2;
    DatOff o{};
    size_t at = 0;
    auto take = [&](size_t n) { const size_t a = at; at += n; return a; };
    o.dw_t = take(ch * 9); o.dw_b = take(ch);
    o.ci_w1 = take(hc * ch); o.ci_b1 = take(hc); o.ci_w2 = take(ch * hc); o.ci_b2 = take(ch);
    o.si_w1 = take(hs * ch); o.si_b1 = take(hs); o.si_w2 = take(hs); o.si_b2 = take(1);
    o.sg_g = take(half); o.sg_b = take(half); o.sg_t = take(half * 9); o.sg_cb = take(half);
    o.temp = take((size_t)net->sw_nh);
    o.total = at;
    return o;
}

extern "C" size_t innfer_dat_block_floats(innfer_net_t net) { return net && net->kind == 8 ? dat_offsets(net).total : 0; }

extern "C" int innfer_dat_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int hidden, int s0, int s1,
                                 int upsampler, int scale, int conv3, const float* h_mean, const int* h_shift) {
    if (!out || !depths) return set_error(INNFER_ERR_INVALID, "dat_create: null argument");
    if (embed_dim < 1 || embed_dim > 256 || num_heads < 2 || num_heads > 8 || (num_heads & 1) || embed_dim % num_heads || embed_dim / num_heads > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: embed_dim=%d num_heads=%d (built: embed_dim <= 256, 2, 4, 6 or 8 heads of <= 32 channels, embed_dim %% num_heads == 0)", embed_dim, num_heads);
    if (embed_dim / 16 < 1) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: embed_dim=%d (built: embed_dim / 8 and embed_dim / 16 in 1 .. 64)", embed_dim);
    if (hidden < 2 || hidden > 1024 || (hidden & 1)) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: a feed-forward of %d hidden channels (built: even, <= 1024)", hidden);
    if (s0 != 8 || (s1 != 32 && s1 != 16)) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: split_size [%d, %d] (built: [8, 32] and [8, 16])", s0, s1);
    if (in_nc < 1 || in_nc > 4 || in_nc != out_nc) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: in_chans=%d, %d output channels (built: equal, 1..4)", in_nc, out_nc);
    if (n_layers < 1 || n_layers > 64) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: %d residual groups", n_layers);
    for (int i = 0; i < n_layers; ++i)
        if (depths[i] < 1 || depths[i] > 64) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: depth %d of residual group %d", depths[i], i);
    if (upsampler < 0 || upsampler > 1) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: upsampler %d (0 pixelshuffle, 1 pixelshuffledirect)", upsampler);
    if (scale < 2 || scale > 4) return set_error(INNFER_ERR_UNSUPPORTED, "dat_create: scale %d (built: 2, 3, 4)", scale);
    innfer_net* net = new innfer_net();
    net->kind = 8; net->in_nc = in_nc; net->out_nc = out_nc; net->nf = 64; net->nb = 0; net->gc = 0; net->scale = scale; net->n_up = 0;
    net->sw_c = embed_dim; net->sw_cp = (embed_dim + 63) / 64 * 64; net->sw_nh = num_heads; net->sw_d = embed_dim / num_heads;
    net->dat_s0 = s0; net->dat_s1 = s1; net->dat_h1p = (hidden / 2 + 63) / 64 * 64;
    net->sw_hid = hidden; net->sw_hp = 2 * net->dat_h1p; net->sw_tail = upsampler; net->sw_conv3 = conv3 != 0;
    net->sw_c4p = (embed_dim / 4 + 63) / 64 * 64;
    net->sw_depths.assign(depths, depths + n_layers);
    const int cp = net->sw_cp;
    for (int p = 0; p < cp / 64; ++p) add_conv(net, "conv_first#" + std::to_string(p), 64, in_nc, true);
    for (int i = 0; i < n_layers; ++i) {
        for (int j = 0; j < depths[i]; ++j) {
            const std::string b = "layers." + std::to_string(i) + ".blocks." + std::to_string(j) + ".";
            swin_add_sliced(net, b + "attn.qkv", (3 * num_heads + 1) / 2 * 64, cp, 1);
            swin_add_sliced(net, b + "attn.proj", cp, 32 * num_heads, 1);
            swin_add_sliced(net, b + "ffn.fc1", net->sw_hp, cp, 1);
            swin_add_sliced(net, b + "ffn.fc2", cp, net->dat_h1p, 1);
            // shifted: the issue's rule, unless the caller names the blocks (a checkpoint's stored masks decide)
            const bool formula = (i % 2 == 0 && j > 0 && (j - 2) % 4 == 0) || (i % 2 != 0 && j % 4 == 0);
            net->dat_shift.push_back(h_shift ? (h_shift[net->nb] != 0) : formula);
            net->dat_aca.push_back(j & 1);
            net->nb++;
        }
        swin_add_resi(net, "layers." + std::to_string(i) + ".conv");
    }
    swin_add_resi(net, "conv_after_body");
    if (upsampler == 1) {
        add_conv(net, "upsample.0", out_nc * scale * scale, cp);
        net->convs.back().Kp = out_nc * scale * scale <= 32 ? 32 : 64;
    } else {
        add_conv(net, "conv_before_upsample.0", 64, cp);
        net->convs.back().slope_ok = true;
        if (scale == 3) add_conv(net, "upsample.0", 576, 64);
        else {
            add_conv(net, "upsample.0", 256, 64); net->convs.back().ps2 = true;
            if (scale == 4) { add_conv(net, "upsample.2", 256, 64); net->convs.back().ps2 = true; net->convs.back().mult = 4.f; }
        }
        add_conv(net, "conv_last", out_nc, 64); net->convs.back().mult = (float)(scale * scale);
    }
    net->sw_ln.assign(2 + 2 * (size_t)net->nb, nullptr);
    net->sw_relb.assign((size_t)net->nb, nullptr);
    net->dat_blk.assign((size_t)net->nb, nullptr);
    net->dat_sib2.assign((size_t)net->nb, 0.f);
    int rc = INNFER_OK;
    {   // x - mean in front of conv_first and nn.LeakyReLU() (slope 0.01) behind conv_before_upsample, as innfer_swinir_create
        float h[8];
        for (int c = 0; c < in_nc; ++c) { h[c] = 1.f; h[in_nc + c] = h_mean ? -h_mean[c] : 0.f; }
        ConvSlot& c0 = net->convs[0];
        if (hipMalloc((void**)&c0.d_map, 2 * in_nc * sizeof(float)) != hipSuccess || hipMemcpy(c0.d_map, h, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = set_error(INNFER_ERR_NOMEM, "dat_create: no device memory for the input map");
        for (size_t i = 0; i < net->convs.size() && rc == INNFER_OK; ++i)
            if (net->convs[i].slope_ok) {
                const std::vector<float> sl(64, 0.01f);
                rc = innfer_net_set_conv_slope(net, (int)i, sl.data());
            }
    }
    if (rc != INNFER_OK) { (void)hipGetLastError(); innfer_net_destroy(net); return rc; }
    *out = net;
    return INNFER_OK;
}

// The per-block parameters of a DAT beside its convs, LayerNorms and bias table: innfer_dat_block_floats(net) host floats in the header's order.  Load time, synchronous.
extern "C" int innfer_net_set_dat_block(innfer_net_t net, int blk, const float* h_params, size_t n_floats) {
    if (!net || !h_params) return set_error(INNFER_ERR_INVALID, "set_dat_block: null argument");
    if (net->kind != 8) return set_error(INNFER_ERR_UNSUPPORTED, "set_dat_block: the network is not a DAT");
    if (blk < 0 || blk >= (int)net->dat_blk.size()) return set_error(INNFER_ERR_INVALID, "set_dat_block: block %d of %zu", blk, net->dat_blk.size());
    const DatOff o = dat_offsets(net);
    if (n_floats != o.total) return set_error(INNFER_ERR_INVALID, "set_dat_block: %zu floats, the block takes %zu (innfer_dat_block_floats)", n_floats, o.total);
    for (size_t i = 0; i < n_floats; ++i)
        if (!std::isfinite(h_params[i])) return set_error(INNFER_ERR_INVALID, "set_dat_block: parameter %zu of block %d is not finite", i, blk);
    if (!net->dat_blk[blk]) INNFER_HIP(hipMalloc((void**)&net->dat_blk[blk], (o.total + 4) * sizeof(float)));
    INNFER_HIP(hipMemcpy(net->dat_blk[blk], h_params, o.total * sizeof(float), hipMemcpyHostToDevice));
    net->dat_sib2[blk] = h_params[o.si_b2];
    return INNFER_OK;
}

// The affine parameters of the GroupNorm behind conv `idx` (RealPLKSR's refine): 64 host floats each, NULL = 1 / 0.  Load time, synchronous.
extern "C" int innfer_net_set_group_norm(innfer_net_t net, int idx, const float* h_gamma, const float* h_beta) {
    if (!net || idx < 0 || idx >= (int)net->convs.size()) return set_error(INNFER_ERR_INVALID, "set_group_norm: bad arguments");
    ConvSlot& c = net->convs[idx];
    if (!c.gn_ok) return set_error(INNFER_ERR_UNSUPPORTED, "set_group_norm: no GroupNorm follows '%s' (built: the refine convs of a RealPLKSR)", c.key.c_str());
    float h[128];
    for (int i = 0; i < 64; ++i) { h[i] = h_gamma ? h_gamma[i] : 1.f; h[64 + i] = h_beta ? h_beta[i] : 0.f; }
    if (!c.d_gn) INNFER_HIP(hipMalloc((void**)&c.d_gn, sizeof h));
    INNFER_HIP(hipMemcpy(c.d_gn, h, sizeof h, hipMemcpyHostToDevice));
    return INNFER_OK;
}

// The activation behind conv `idx` of an SRVGGNetCompact as K per-channel slopes (host floats): y = x >= 0 ? x : slope[c] * x -- nn.PReLU's weight, or the
// constant 0 (ReLU) / 0.1 (LeakyReLU(0.1)).  Load time, synchronous, like innfer_net_set_conv.
extern "C" int innfer_net_set_conv_slope(innfer_net_t net, int idx, const float* h_slope) {
    if (!net || idx < 0 || idx >= (int)net->convs.size() || !h_slope) return set_error(INNFER_ERR_INVALID, "set_conv_slope: bad arguments");
    ConvSlot& c = net->convs[idx];
    if (!c.slope_ok) return set_error(INNFER_ERR_UNSUPPORTED, "set_conv_slope: '%s' has no per-channel activation (built: the convs of an SRVGGNetCompact except its last)", c.key.c_str());
    const int per = 16 * conv_nt_for(c.K);
    const size_t n = (size_t)((c.K + per - 1) / per) * per;
    std::vector<float> h(n, 0.f);
    for (int k = 0; k < c.K; ++k) h[k] = h_slope[k];
    if (!c.d_slope) INNFER_HIP(hipMalloc((void**)&c.d_slope, n * sizeof(float)));
    INNFER_HIP(hipMemcpy(c.d_slope, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return INNFER_OK;
}

extern "C" int innfer_net_set_outm(innfer_net_t net, int outm) {
    if (!net || outm < 0 || outm > 4) return set_error(INNFER_ERR_INVALID, "set_outm: 0 none, 1 scaltanh, 2 tanh, 3 sigmoid, 4 clamp");
    net->outm = outm;
    return INNFER_OK;
}

extern "C" void innfer_net_destroy(innfer_net_t net) {
    if (!net) return;
    for (float* q : net->sw_ln) if (q) (void)hipFree(q);
    for (float* q : net->sw_relb) if (q) (void)hipFree(q);
    for (float* q : net->sw_tau) if (q) (void)hipFree(q);
    for (float* q : net->hat_ca) if (q) (void)hipFree(q);
    for (float* q : net->dat_blk) if (q) (void)hipFree(q);
    for (auto& c : net->convs) {
        if (c.d_w) (void)hipFree(c.d_w);
        if (c.d_b) (void)hipFree(c.d_b);
        if (c.d_w32) (void)hipFree(c.d_w32);
        if (c.d_fuse) (void)hipFree(c.d_fuse);
        if (c.d_up4) (void)hipFree(c.d_up4);
        if (c.d_up4p) (void)hipFree(c.d_up4p);
        if (c.d_ps) (void)hipFree(c.d_ps);
        if (c.d_bps) (void)hipFree(c.d_bps);
        if (c.d_b4) (void)hipFree(c.d_b4);
        if (c.d_map) (void)hipFree(c.d_map);
        if (c.d_slope) (void)hipFree(c.d_slope);
        if (c.d_gn) (void)hipFree(c.d_gn);
    }
    delete net;
}

extern "C" int innfer_net_num_convs(innfer_net_t net) { return net ? (int)net->convs.size() : INNFER_ERR_INVALID; }
extern "C" int innfer_net_scale(innfer_net_t net) { return net ? net->scale : INNFER_ERR_INVALID; }

extern "C" int innfer_net_conv_info(innfer_net_t net, int idx, char* key, size_t key_cap, int* K, int* C) {
    if (!net || idx < 0 || idx >= (int)net->convs.size()) return set_error(INNFER_ERR_INVALID, "conv_info: bad index %d", idx);
    const ConvSlot& c = net->convs[idx];
    if (key && key_cap) { strncpy(key, c.key.c_str(), key_cap - 1); key[key_cap - 1] = 0; }
    if (K) *K = c.K;
    if (C) *C = c.C;
    return INNFER_OK;
}

// The (wl | wh | wh) panels of one loaded conv for the fp32-accurate mode (conv_pack_split), from the fp32 weights kept at innfer_net_set_conv.
static int build_split_panels(ConvSlot& c) {
    std::vector<char> host(3 * (c.ksize == 1 ? conv_packed_bytes_taps(c.K, c.C, TAPS_1X1) : conv_packed_bytes(c.K, c.C)));
    if (c.ksize == 1) conv_pack_1x1_split(c.h_w.data(), c.K, c.C, host.data());
    else conv_pack_split(c.h_w.data(), c.K, c.C, host.data());
    if (hipMalloc(&c.d_w32, host.size()) != hipSuccess) {
        c.d_w32 = nullptr; (void)hipGetLastError();
        return set_error(INNFER_ERR_NOMEM, "out of device memory for the fp32-accurate panels of '%s' (%zu bytes)", c.key.c_str(), host.size());
    }
    if (hipMemcpy(c.d_w32, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(c.d_w32); c.d_w32 = nullptr; (void)hipGetLastError();
        return set_error(INNFER_ERR_HIP, "copying the fp32-accurate panels of '%s' failed", c.key.c_str());
    }
    return INNFER_OK;
}

// A first conv's weights as first_conv_mfma reads them (FirstConvLaunch.w): OIHW [K][C][3][3] -> k-major [C * 9][K] fp32.  The one layout code of
// innfer_net_set_conv and innfer_first_conv.
static void first_conv_layout(const float* w, int K, int C, float* d) {
    for (int ci = 0; ci < C; ++ci)
        for (int t = 0; t < 9; ++t)
            for (int k = 0; k < K; ++k) d[((size_t)ci * 9 + t) * K + k] = w[((size_t)k * C + ci) * 9 + t];
}

extern "C" int innfer_net_set_conv(innfer_net_t net, int idx, const float* w, const float* b) {
    if (!net || idx < 0 || idx >= (int)net->convs.size() || !w) return set_error(INNFER_ERR_INVALID, "set_conv: bad arguments");
    ConvSlot& c = net->convs[idx];
    std::vector<char> host;
    size_t bias_n;
    if (c.first && net->unshuffle > 1) {          // the LDS image of conv_first_unshuffle.hip: hi | lo fragments, k in window order
        host.resize(first_unshuffle_packed_bytes(c.K, net->unshuffle));
        first_unshuffle_pack(w, c.K, net->unshuffle, host.data());
        bias_n = c.K;
    } else if (c.first) {
        host.resize((size_t)c.C * 9 * c.K * sizeof(float));
        first_conv_layout(w, c.K, c.C, (float*)host.data());
        bias_n = c.K;
    } else if (c.plk) {              // RealPLKSR's lk.conv [16, 16, k, k]: the streamed [step][lane][8] panel of plk_conv.hip
        host.resize(plk_packed_bytes(c.ksize));
        plk_pack(w, c.ksize, host.data());
        bias_n = 16;
    } else {
        if (c.ksize == 1) {          // [K,C,1,1]: the one-tap panel of the kernel's 1x1 instantiation
            host.resize(conv_packed_bytes_taps(c.K, c.C, TAPS_1X1));
            conv_pack_1x1(w, c.K, c.C, host.data());
        } else if (c.Kp) {           // SRVGGNetCompact's last conv: K valid rows of a 32- / 64-output panel, the rest zero
            std::vector<float> wp((size_t)c.Kp * c.C * 9, 0.f);
            std::copy(w, w + (size_t)c.K * c.C * 9, wp.begin());
            host.resize(conv_packed_bytes(c.Kp, c.C));
            c.rowp = c.Kp == 64;
            conv_pack(wp.data(), c.Kp, c.C, host.data(), c.rowp);
        } else {
            host.resize(conv_packed_bytes(c.K, c.C));
            c.rowp = c.K == 64 && !c.lane_rows;
            conv_pack(w, c.K, c.C, host.data(), c.rowp);
        }
        const int per = 16 * conv_nt_for(c.Kp ? c.Kp : c.K);
        bias_n = (size_t)(((c.Kp ? c.Kp : c.K) + per - 1) / per) * per;
        c.h_w.assign(w, w + (size_t)c.K * c.C * c.ksize * c.ksize);
        if (c.d_w32) { (void)hipFree(c.d_w32); c.d_w32 = nullptr; }
        if (c.up2x && c.ksize == 3 && c.K % 64 == 0 && c.C % 32 == 0) {
            // nearest-2x + conv3x3 (block.py:358) == ConvTranspose2d(4, 2, 1) with the taps that meet the same LR pixel summed (conv_pack_up2x_phases)
            std::vector<char> pk(conv_packed_bytes_deconv2x(c.K, c.C));
            conv_pack_up2x_phases(w, c.K, c.C, pk.data());
            std::vector<float> b4((size_t)4 * c.K, 0.f);
            if (b) for (int ph = 0; ph < 4; ++ph) for (int k = 0; k < c.K; ++k) b4[(size_t)ph * c.K + k] = b[k];
            if (!c.d_up4) INNFER_HIP(hipMalloc(&c.d_up4, pk.size()));
            if (!c.d_b4) INNFER_HIP(hipMalloc((void**)&c.d_b4, b4.size() * sizeof(float)));
            INNFER_HIP(hipMemcpy(c.d_up4, pk.data(), pk.size(), hipMemcpyHostToDevice));
            if (c.rowp && c.C == 64) {
                conv_pack_up2x_phases(w, c.K, c.C, pk.data(), 1);
                if (!c.d_up4p) INNFER_HIP(hipMalloc(&c.d_up4p, pk.size()));
                INNFER_HIP(hipMemcpy(c.d_up4p, pk.data(), pk.size(), hipMemcpyHostToDevice));
            }
            INNFER_HIP(hipMemcpy(c.d_b4, b4.data(), b4.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (c.ps2 && c.ksize == 3 && c.K % 256 == 0 && c.C % 32 == 0) {
            std::vector<char> pk(conv_packed_bytes(c.K, c.C));
            std::vector<float> bp(c.K, 0.f);
            conv_pack_shuffle2(w, b, c.K, c.C, pk.data(), bp.data());
            if (!c.d_ps) INNFER_HIP(hipMalloc(&c.d_ps, pk.size()));
            if (!c.d_bps) INNFER_HIP(hipMalloc((void**)&c.d_bps, bp.size() * sizeof(float)));
            INNFER_HIP(hipMemcpy(c.d_ps, pk.data(), pk.size(), hipMemcpyHostToDevice));
            INNFER_HIP(hipMemcpy(c.d_bps, bp.data(), bp.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (c.ksize == 3 && c.C == 64 && c.K <= 3) {          // (only the network's last conv has this shape)
            std::vector<char> fp(4096);
            conv_pack_fuse_last(w, c.K, fp.data(), 1);          // (fused behind HR_conv0, a 64-output conv: its row order)
            if (!c.d_fuse) INNFER_HIP(hipMalloc(&c.d_fuse, fp.size()));
            INNFER_HIP(hipMemcpy(c.d_fuse, fp.data(), fp.size(), hipMemcpyHostToDevice));
        }
    }
    std::vector<float> bias(bias_n, 0.f);
    if (b) for (int k = 0; k < c.K; ++k) bias[k] = b[k];
    if (!c.d_w) INNFER_HIP(hipMalloc(&c.d_w, host.size()));
    if (!c.d_b) INNFER_HIP(hipMalloc((void**)&c.d_b, bias_n * sizeof(float)));
    INNFER_HIP(hipMemcpy(c.d_w, host.data(), host.size(), hipMemcpyHostToDevice));
    INNFER_HIP(hipMemcpy(c.d_b, bias.data(), bias_n * sizeof(float), hipMemcpyHostToDevice));
    c.loaded = true;
    // a network already in the fp32-accurate mode (set_precision(1) before this set_conv, or one conv re-set afterwards: the ABI-106 call order) gets this
    // conv's split panels here -- set_conv is a load-time call like set_precision; innfer_net_forward never allocates
    if (net->fp32 && !c.first) return build_split_panels(c);
    return INNFER_OK;
}

extern "C" int innfer_net_set_conv_input_map(innfer_net_t net, int idx, const float* alpha, const float* shift, int act) {
    if (!net || idx < 0 || idx >= (int)net->convs.size() || act < 0 || act > 2) return set_error(INNFER_ERR_INVALID, "set_conv_input_map: bad arguments");
    ConvSlot& c = net->convs[idx];
    if (!alpha && !shift && act == 0) {          // no map
        if (c.d_map) { (void)hipFree(c.d_map); c.d_map = nullptr; }
        c.map_act = 0;
        return INNFER_OK;
    }
    if (!c.map_ok)
        return set_error(INNFER_ERR_UNSUPPORTED, "set_conv_input_map: '%s' (built in front of the first conv of an SRResNet block and of LR_conv of either network)", c.key.c_str());
    std::vector<float> h(2 * (size_t)c.C);
    for (int i = 0; i < c.C; ++i) { h[i] = alpha ? alpha[i] : 1.f; h[c.C + i] = shift ? shift[i] : 0.f; }
    if (!c.d_map) INNFER_HIP(hipMalloc((void**)&c.d_map, h.size() * sizeof(float)));
    INNFER_HIP(hipMemcpy(c.d_map, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    c.map_act = act;
    return INNFER_OK;
}

// fp32 = 1: the forward keeps fp32 accuracy -- every activation is a pair of fp16 slabs (hi, lo = (x - hi) * 2^11: 22 significant bits), every weight a
// pair of panels, products are xh wh + 2^-11 (xh wl + xl wh) on the fp16 MFMA path with fp32 accumulation (conv3x3.hip, SPLIT): three times the MFMA
// work and twice the bytes of the fp16 forward.  The reference's fp32 mode on the GPU (`-no_fp16`: run.py:345,421-422).
extern "C" int innfer_net_set_precision(innfer_net_t net, int fp32) {
    if (!net || (fp32 != 0 && fp32 != 1)) return set_error(INNFER_ERR_INVALID, "set_precision: 0 (fp16 arithmetic) or 1 (fp32-accurate)");
    if (fp32 && net->kind == 2) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: SRVGGNetCompact is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 3) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: SPAN is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 4) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: RealPLKSR is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 5) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: SwinIR is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 6) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: HAT is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 7) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: Swin2SR is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 8) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: DAT is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32 && net->kind == 9) return set_error(INNFER_ERR_UNSUPPORTED, "set_precision: DRCT is built for the fp16 mode only (no fp32-accurate engine)");
    if (fp32) {
        // The (wl | wh | wh) panels of every loaded conv are built HERE -- a load-time call, with its hipMalloc and synchronous copies -- never inside
        // innfer_net_forward (stream capture, concurrent callers).  Idempotent: a conv that already has its panels is skipped; innfer_net_set_conv
        // drops a conv's panels, so the call after a weight change rebuilds exactly those.
        std::vector<ConvSlot*> built;              // panels allocated by THIS call: released again when one of them does not fit
        for (auto& c : net->convs) {
            if (c.first || c.d_w32 || !c.loaded) continue;
            const int rc = build_split_panels(c);
            if (rc != INNFER_OK) {
                for (ConvSlot* q : built) { (void)hipFree(q->d_w32); q->d_w32 = nullptr; }
                return rc;
            }
            built.push_back(&c);
        }
    }
    net->fp32 = fp32;
    return INNFER_OK;
}

extern "C" int innfer_net_set_band_rows(innfer_net_t net, int rows) {
    if (!net || rows < 0) return set_error(INNFER_ERR_INVALID, "set_band_rows: bad arguments");
    net->band_rows = rows;
    return INNFER_OK;
}

extern "C" int innfer_net_set_upconv_phases(innfer_net_t net, int on) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_upconv_phases: null network");
    if (on < 0 || on > 2) return set_error(INNFER_ERR_INVALID, "set_upconv_phases: 0 (nine taps on the HR grid), 1 (four phases, one visit of a tile: default) or 2 (one phase per visit)");
    net->up_phases = on;
    return INNFER_OK;
}

extern "C" int innfer_net_set_residual_lds(innfer_net_t net, int on) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_residual_lds: null network");
    if (on < 0 || on > 2) return set_error(INNFER_ERR_INVALID, "set_residual_lds: 0 (epilogue loads), 1 (the RRDB-end layers: default) or 2 (every dense block)");
    net->res_lds = on;
    return INNFER_OK;
}

extern "C" int innfer_net_set_consumer_grid(innfer_net_t net, int mode) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_consumer_grid: null network");
    if (mode < 0 || mode > 1) return set_error(INNFER_ERR_INVALID, "set_consumer_grid: 1 (2 x 4 consumer grid with the residual prefetch: default) or 0 (the 8 x 1 form)");
    net->consumer_grid = mode;
    return INNFER_OK;
}

extern "C" int innfer_net_set_fused_tail(innfer_net_t net, int on) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_fused_tail: null network");
    net->fused_tail = on ? 1 : 0;
    return INNFER_OK;
}

extern "C" int innfer_net_set_hr_chain(innfer_net_t net, int on) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_hr_chain: null network");
    net->hr_chain = on ? 1 : 0;
    return INNFER_OK;
}

extern "C" int innfer_net_set_u8_io(innfer_net_t net, int normalize, int fp16_mode) {
    if (!net) return set_error(INNFER_ERR_INVALID, "set_u8_io: null net");
    net->u8_normalize = normalize != 0;
    net->u8_round16 = fp16_mode != 0;
    return INNFER_OK;
}

extern "C" int innfer_net_set_final_act(innfer_net_t net, int act) {
    if (!net || (act != 0 && act != 1 && act != 2 && act != 3 && act != 6))
        return set_error(INNFER_ERR_INVALID, "set_final_act: act %d (0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 tanh, 6 sigmoid)", act);
    net->final_act = act;
    return INNFER_OK;
}

extern "C" double innfer_net_flops(innfer_net_t net, int N, int H, int W) {
    if (!net) return 0.0;
    if (net->kind == 5 || net->kind == 7) {        // SwinIR, Swin2SR: every conv on the padded grid (its tail's at their own resolution) + the two products of every window and head
        const double px = (double)N * ((H + 7) / 8 * 8) * ((W + 7) / 8 * 8);
        double f = (double)net->nb * net->sw_nh * (px / 64) * 4.0 * 64 * 64 * 32;
        for (auto& c : net->convs) f += 2.0 * c.ksize * c.ksize * c.K * c.C * px * c.mult;
        return f;
    }
    if (net->kind == 6) {        // HAT: as SwinIR on the grid padded to 16; 256 x 256 scores per window and head in a HAB, 256 x 576 in an OCAB
        const double px = (double)N * ((H + 15) / 16 * 16) * ((W + 15) / 16 * 16);
        double f = net->sw_nh * (px / 256) * 4.0 * 256 * 32 * (256.0 * net->nb + 576.0 * net->sw_depths.size());
        for (auto& c : net->convs) f += 2.0 * c.ksize * c.ksize * c.K * c.C * px * c.mult;
        return f;
    }
    if (net->kind == 9) {        // DRCT: as HAT's grid; per block the two products of every window and head on its real head width
        const double px = (double)N * ((H + 15) / 16 * 16) * ((W + 15) / 16 * 16);
        double f = 0.0;
        for (size_t b = 0; b < net->dr_nh.size(); ++b) f += (px / 256) * 4.0 * 256 * 256 * (net->sw_c + 32.0 * (b % 5));
        for (auto& c : net->convs) f += 2.0 * c.ksize * c.ksize * c.K * c.C * px * c.mult;
        return f;
    }
    if (net->kind == 8) {        // DAT: every conv on the grid itself; per even block the two products of every window and head on the frame padded to s1, per odd block the Gram and the apply
        const double px = (double)N * H * W, s1 = net->dat_s1, T = (double)net->dat_s0 * s1;
        const double pxp = (double)N * std::ceil(H / s1) * s1 * std::ceil(W / s1) * s1;
        double f = 0.0;
        for (size_t b = 0; b < net->dat_blk.size(); ++b) f += net->sw_nh * (net->dat_aca[b] ? px * 4.0 * 32 * 32 : (pxp / T) * 4.0 * T * T * 32);
        for (auto& c : net->convs) f += 2.0 * c.ksize * c.ksize * c.K * c.C * px * c.mult;
        return f;
    }
    H = (H + net->unshuffle - 1) / net->unshuffle; W = (W + net->unshuffle - 1) / net->unshuffle;      // the LR grid
    double px = (double)N * H * W, f = 0.0;
    const int nconv = (int)net->convs.size();
    // resolution multiplier per conv: trunk at 1x, up-conv u at 4^(u+1) (RRDB: conv runs AFTER the
    // upsample; SRGAN: conv runs BEFORE the shuffle, i.e. at 4^u), tail convs at scale^2.
    for (int i = 0; i < nconv; ++i) {
        const ConvSlot& c = net->convs[i];
        double mult = 1.0;
        const int tail0 = nconv - 2 - net->n_up;          // first up conv
        if (i >= tail0) {
            const int u = i - tail0;
            const double f2 = net->scale == 3 ? 9.0 : 4.0;     // pixels per input pixel after one upsample stage
            if (u < net->n_up) mult = std::pow(f2, !net->ps_up ? u + 1 : u);
            else mult = std::pow(f2, net->n_up);
        }
        f += 2.0 * c.ksize * c.ksize * c.K * c.C * px * mult;
    }
    return f;
}

// Workspace carve (all fp16 NHWC):
//   fea        [N,H,W,nf]               conv_first output, kept for the trunk shortcut
//   slab[3]    [N,H,W,nf+4gc]           rotating RDB slabs (RRDB) / ping-pong features (SRGAN)
//   trunk      [N,H,W,nf]
//   up[u]      [N,2^(u+1)H,2^(u+1)W,nf] after each upsample stage
//   hr         [N,sH,sW,nf]             HR_conv0 output
struct Carve {
    size_t fea, slab[3], trunk, up[5], hr, tmp, total;
    size_t lo;                   // fp32-accurate mode: every buffer's lo twin lies `lo` bytes behind it (the second half of the workspace)
    int slab_w;
};

// SwinIR's workspace (kind 5) on the padded grid Hp x Wp: the padded input, the first conv's result (the last shortcut), two buffers the residual groups alternate between,
// the token stream, the normalised tokens, the qkv slab (head-padded), the attention's result (head-padded), the MLP's hidden slab, the two C / 4 buffers of '3conv',
// the tail's slabs, and the full-size result in front of the crop.
// HAT (kind 6) pads to multiples of 16 and adds the conv block's 64-channel slab, its C_pad-channel result z, the channel attention's vector and the segment sums.
struct SwinCarve { size_t xin, f0, r[2], t, u, qkv, att, hid, c4[2], b64, up[2], hr, outp, zc, z, y, pool, gram, amat, total; int Hp, Wp; };
static SwinCarve swin_carve(const innfer_net* net, int N, int H, int W) {
    SwinCarve c{};
    const int wsz = net->kind == 6 || net->kind == 9 ? 16 : net->kind == 8 ? 1 : 8;          // (DAT works on H x W itself)
    c.Hp = (H + wsz - 1) / wsz * wsz; c.Wp = (W + wsz - 1) / wsz * wsz;
    const size_t px = (size_t)N * c.Hp * c.Wp, s2 = (size_t)net->scale * net->scale;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    c.xin = take(px * net->in_nc * 2);
    c.f0 = take(px * net->sw_cp * 2);
    if (net->kind == 9) {        // DRCT: r[] are the two dense slabs (x | x1 .. x4 and one spare group, an even count), t and u the widest block's tokens; qkv / att / hid: the maximum over the blocks
        const DrctDims dd = drct_dims(net);
        c.r[0] = take(px * 32 * dd.dense_groups * 2); c.r[1] = take(px * 32 * dd.dense_groups * 2);
        c.t = take(px * dd.lp[4] * 2);
        c.u = take(px * dd.lp[4] * 2);
        c.qkv = take(px * (size_t)dd.max_sq * 64 * 2);
        c.att = take(px * (size_t)dd.max_hg * 32 * 2);
        c.hid = take(px * (size_t)dd.max_hp * 2);
    } else {
    c.r[0] = take(px * net->sw_cp * 2); c.r[1] = take(px * net->sw_cp * 2);
    c.t = take(px * net->sw_cp * 2);
    c.u = take(px * net->sw_cp * 2);
    c.qkv = take(px * ((3 * net->sw_nh + 1) / 2 * 64) * 2);
    c.att = take(px * 32 * net->sw_nh * 2);
    c.hid = take(px * net->sw_hp * 2);
    }
    if (net->sw_conv3) { c.c4[0] = take(px * net->sw_c4p * 2); c.c4[1] = take(px * net->sw_c4p * 2); }
    if (net->sw_tail == 1) c.hr = take(px * net->convs.back().Kp * 2);
    else {
        c.b64 = take(px * 64 * 2);
        if (net->sw_tail == 0 && net->scale == 3) { c.up[0] = take(px * 576 * 2); c.up[1] = take(px * 9 * 64 * 2); }
        else { c.up[0] = take(px * 4 * 64 * 2); if (net->scale == 4) c.up[1] = take(px * 16 * 64 * 2); }
        if (net->sw_tail == 2) c.hr = take(px * s2 * 64 * 2);
    }
    c.outp = take(px * s2 * net->out_nc * 4);
    if (net->kind == 6) {
        c.zc = take(px * 64 * 2);
        c.z = take(px * net->sw_cp * 2);
        c.y = take((size_t)N * net->sw_cp * 4);
        c.pool = take(ca_work_floats(N, (long)c.Hp * c.Wp, net->sw_cp) * 4);
    }
    if (net->kind == 8) {        // DAT: c = GELU(dwconv(v)) (head-padded), the normalised second half of the feed-forward, the per-channel gate, the pool's and the Gram's segment records, A
        c.z = take(px * 32 * net->sw_nh * 2);
        c.zc = take(px * net->dat_h1p * 2);
        c.y = take((size_t)N * 32 * net->sw_nh * 4);
        c.pool = take(ca_work_floats(N, (long)H * W, 32 * net->sw_nh) * 4);
        c.gram = take(csa_work_floats(N, (long)H * W, net->sw_nh) * 4);
        c.amat = take((size_t)N * net->sw_nh * 1024 * 4);
    }
    c.total = off;
    return c;
}

static Carve carve(const innfer_net* net, int N, int H, int W) {
    Carve c{};
    if (net->kind == 5 || net->kind == 6 || net->kind == 7 || net->kind == 8 || net->kind == 9) { c.total = swin_carve(net, N, H, W).total; return c; }
    const size_t px = (size_t)N * H * W;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    if (net->kind == 2) {        // SRVGGNetCompact: the two ping-pong feature slabs (one when there is no nf -> nf conv) and the last conv's 32- / 64-channel slab
        size_t off = 0;
        c.slab_w = net->nf;
        c.slab[0] = off; off += al(px * net->nf * 2);
        c.slab[1] = off; if (net->nb > 0) off += al(px * net->nf * 2);
        c.hr = off; off += al(px * net->convs.back().Kp * 2);
        c.total = off;
        return c;
    }
    if (net->kind == 3) {        // SPAN: the concat slab (f0 | conv_2 | b1 | b5_2, nf channels each), three rotating feature slabs, the upsampler's 32- / 64-channel slab
        size_t off = 0;
        c.slab_w = net->nf;
        c.fea = off; off += al(px * 4 * net->nf * 2);
        for (int i = 0; i < 3; ++i) { c.slab[i] = off; off += al(px * net->nf * 2); }
        c.hr = off; off += al(px * net->convs.back().Kp * 2);
        c.total = off;
        return c;
    }
    if (net->kind == 4) {        // RealPLKSR: x (64 channels; norm + skip rewrites it in place), the Mish slab (128 channels; its first half later holds the gated tensor,
                                 // its second refine's result), three groups [U0 | T0 | U1] around the large-kernel conv, the last conv's slab, the GroupNorm records and affine
        size_t off = 0;
        c.slab_w = net->nf;
        c.fea = off; off += al(px * 64 * 2);
        c.slab[0] = off; off += al(px * 128 * 2);
        c.slab[1] = off; off += al(px * 96 * 2);
        c.hr = off; off += al(px * net->convs.back().Kp * 2);
        c.tmp = off; off += al(gn_work_floats(N, (long)H * W) * sizeof(float));
        c.total = off;
        return c;
    }
    c.slab_w = net->kind == 0 ? net->nf + 4 * net->gc : net->nf;
    size_t off = 0;
    c.fea = off; off += al(px * net->nf * 2);
    for (int i = 0; i < 3; ++i) { c.slab[i] = off; off += al(px * c.slab_w * 2); }
    c.trunk = off; off += al(px * net->nf * 2);
    c.tmp = off; if (net->plus) off += al(px * net->gc * 2);          // conv1x1(x) of the current RDB
    size_t m = 1;
    for (int u = 0; u < net->n_up; ++u) { m *= net->scale == 3 ? 9 : 4; c.up[u] = off; off += al(px * m * net->nf * 2); }
    c.hr = off; off += al(px * m * net->nf * 2);
    c.lo = net->fp32 ? off : 0;
    c.total = net->fp32 ? 2 * off : off;
    return c;
}

extern "C" size_t innfer_net_workspace_bytes(innfer_net_t net, int N, int H, int W) {
    if (!net || N <= 0 || H <= 0 || W <= 0) return 0;
    return carve(net, N, (H + net->unshuffle - 1) / net->unshuffle, (W + net->unshuffle - 1) / net->unshuffle).total;
}

namespace {

// Optional per-launch timing (innfer_net_forward_timed): HIP events on the launch stream
// bracket every kernel of one forward.
struct LaunchTimer {
    std::vector<hipEvent_t> ev;      // 2 per launch
    std::vector<double> flops;
    std::vector<double> bytes;       // algorithmic HBM bytes of the launch: every operand read once, every result written once
    std::vector<int> kind;           // 0 first conv; 16*NT + out_mode (+ 1000 / 2000 / 3000: see do_conv) for the MFMA convs
};
thread_local LaunchTimer* g_timer = nullptr;

int timed_begin(hipStream_t s) {
    if (!g_timer) return INNFER_OK;
    hipEvent_t e;
    INNFER_HIP(hipEventCreate(&e));
    INNFER_HIP(hipEventRecord(e, s));
    g_timer->ev.push_back(e);
    return INNFER_OK;
}

int timed_end(hipStream_t s, double flops, double bytes, int kind) {
    if (!g_timer) return INNFER_OK;
    hipEvent_t e;
    INNFER_HIP(hipEventCreate(&e));
    INNFER_HIP(hipEventRecord(e, s));
    g_timer->ev.push_back(e);
    g_timer->flops.push_back(flops);
    g_timer->bytes.push_back(bytes);
    g_timer->kind.push_back(kind);
    return INNFER_OK;
}

// INNFER_DEBUG=1: print every launch and synchronise after it (fault localisation only).
bool debug_sync() {
    static const bool on = getenv("INNFER_DEBUG") != nullptr;
    return on;
}

int debug_after(const char* what, hipStream_t s) {
    if (!debug_sync()) return INNFER_OK;
    fprintf(stderr, "[innfer] %s ... ", what); fflush(stderr);
    hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "%s\n", hipGetErrorString(e)); fflush(stderr);
    return e == hipSuccess ? INNFER_OK : set_error(INNFER_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

int do_conv(const ConvLaunch& L, hipStream_t s) {
    int rc = timed_begin(s);
    if (rc) return rc;
    if (debug_sync())
        fprintf(stderr, "[innfer] conv C=%d K=%d N=%d H=%d W=%d up=%d act=%d mode=%d rows=[%d,%d) in_g=%ld out_g=%ld\n",
                L.C, L.K, L.N, L.H, L.W, L.up, L.act, L.out_mode, L.y0, L.y1, L.in_gstride, L.out_gstride);
    {
        // whole-frame launches alternate their traversal direction (Infinity Cache reuse between layers)
        const bool alt = INNFER_KNOB("INNFER_TILE_REV", 1) != 0;
        thread_local unsigned parity = 0;
        ConvLaunch R = L;
        const int y1 = L.y1 > 0 ? L.y1 : L.H;
        R.rev = (alt && L.y0 == 0 && y1 == L.H) ? (int)(parity++ & 1) : 0;
        rc = conv_launch(R, s);
    }
    if (rc) return rc;
    rc = debug_after("conv3x3", s);
    if (rc) return rc;
    const int y1 = L.y1 > 0 ? L.y1 : L.H;
    const double px = (double)L.N * (y1 - L.y0) * L.W;
    const int taps = L.conv1x1 ? 1 : 9;
    // algorithmic bytes per output pixel: C input channels (a quarter of them per pixel behind the folded nearest-2x), K outputs, K per residual
    const double obytes = L.out_mode == OUT_NCHW ? (L.out_u8 ? 1.0 : L.out_f32 ? 4.0 : 2.0) : 2.0;
    const double bytes = px * (L.C * 2.0 / (L.up ? 4.0 : 1.0) + L.K * obytes + (L.res1 ? L.K * 2.0 : 0.0) + (L.res2 ? L.K * 2.0 : 0.0))
                         + (double)taps * L.K * L.C * 2.0;
    if (L.fuse_w) {      // HR_conv0 + conv_last as one launch (+ the rim pass): both convs' FLOPs; bytes: C channels in, the planar result out, both weight sets
        const double ob = L.fuse_out_mode == 2 ? 1.0 : L.fuse_out_mode == 1 ? 4.0 : 2.0;
        return timed_end(s, 2.0 * 9.0 * (L.K * (double)L.C + 64.0 * L.fuse_oc) * px, px * (L.C * 2.0 + L.fuse_oc * ob) + 9.0 * (L.K * L.C + 64.0 * L.fuse_oc) * 2.0, 2000 + 16 * conv_nt_for(L.K) + L.out_mode);
    }
    // launch kinds: 16 * NT + out_mode, + 1000 fp32-accurate (split) form, + 2000 fused HR_conv0 + conv_last (TMF TAPS_3X3 | PC_FUSE), + 3000 the four 2x2-tap phases
    // of an upconv_block (TM TAPS_PHASE, K = 4 * phase_c on the LR grid), + 4000 the PixelShuffle(2) store on the producer / consumer kernel (TMF TAPS_3X3 | PC_ROWP | PC_PSH): their own
    // instantiations, their own rows in the bench's per-kernel table.
    // The phase form's FLOPs are the ALGORITHMIC ones of the layer it replaces (nine taps on the 2H x 2W grid = 2 * 9 * 4K * C per LR pixel); it executes 4/9 of them.
    // (fp32-accurate mode: the same algorithmic FLOPs -- executed: 3x --, two slabs per tensor, three panels per weight)
    return timed_end(s, 2.0 * taps * L.K * L.C * px, L.split ? 2.0 * bytes + (double)taps * L.K * L.C * 2.0 : bytes,
                     16 * conv_nt_for(L.K) + L.out_mode + (L.split ? 1000 : 0) + (L.deconv_phases ? 3000 : 0) + ((L.out_mode == OUT_SHUFFLE2 && L.rowp == 2) ? 4000 : 0));
}

// nearest-neighbour upsampling of a slab by an integer factor (src = dst / f, block.py:321-322).  The 2x case is folded into the conv's input
// addressing; the 3x models (one stage, RRDBNet_arch.py:33-36) materialise the tensor: a tile's source columns are not a fixed function of
// the column inside the tile when the tile width (32) is not a multiple of the factor.  One thread per (output pixel, 16-byte piece).
__global__ void slab_upsample_nearest(const f16* src, long src_g, f16* dst, long dst_g, int groups, int N, int H, int W, int f) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int HO = H * f, WO = W * f;
    const long M = (long)N * HO * WO;
    if (i >= M * 4 * groups) return;
    const int q = (int)(i & 3);
    const long r = i >> 2;
    const int g = (int)(r / M);
    const long m = r - g * M;
    const int X = (int)(m % WO), Y = (int)((m / WO) % HO);
    const long n = m / ((long)WO * HO);
    const long sp = (n * H + Y / f) * W + X / f;
    *(f16x8*)(dst + g * dst_g + m * 32 + q * 8) = *(const f16x8*)(src + g * src_g + sp * 32 + q * 8);
}

// Input map of a 'NAC' conv block: dst = act(alpha[c] * src + shift[c]) on a slab (8 channels per thread)
__global__ void slab_input_map(const f16* src, f16* dst, long g_elems, int groups, const float* map, int C, int act) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = g_elems / 8;
    if (i >= per * groups) return;
    const int g = (int)(i / per);
    const long r = i % per;
    const int c = g * 32 + (int)(r & 3) * 8;
    const f16x8 x = *(const f16x8*)(src + g * g_elems + r * 8);
    f16x8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = c + e < C ? (float)x[e] * map[c + e] + map[C + c + e] : 0.f;
        if (act == 1) v = fmaxf(v, 0.2f * v);
        else if (act == 2) v = fmaxf(v, 0.f);
        y[e] = (f16)v;
    }
    *(f16x8*)(dst + g * g_elems + r * 8) = y;
}

// The same on the (hi, lo) slab pairs of the fp32-accurate mode: x = hi + lo * 2^-11, mapped in fp32, split again
__global__ void slab_input_map_split(const f16* src, f16* dst, long lo, long g_elems, int groups, const float* map, int C, int act) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = g_elems / 8;
    if (i >= per * groups) return;
    const int g = (int)(i / per);
    const long r = i % per;
    const int c = g * 32 + (int)(r & 3) * 8;
    const f16x8 xh = *(const f16x8*)(src + g * g_elems + r * 8), xl = *(const f16x8*)(src + lo + g * g_elems + r * 8);
    f16x8 yh, yl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = __builtin_fmaf((float)xl[e], 1.0f / 2048.0f, (float)xh[e]);
        float v = c + e < C ? x * map[c + e] + map[C + c + e] : 0.f;
        if (act == 1) v = fmaxf(v, 0.2f * v);
        else if (act == 2) v = fmaxf(v, 0.f);
        yh[e] = (f16)v;
        yl[e] = (f16)((v - (float)yh[e]) * 2048.0f);
    }
    *(f16x8*)(dst + g * g_elems + r * 8) = yh;
    *(f16x8*)(dst + lo + g * g_elems + r * 8) = yl;
}

// PixelShuffle(r) between slabs: out[n, y r + i, x r + j, c] = in[n, y, x, c r^2 + i r + j] (torch.nn.PixelShuffle); 8 output channels per thread
__global__ void slab_pixel_shuffle(const f16* src, long src_g, f16* dst, long dst_g, int nf, int N, int H, int W, int r) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = nf / 8, WO = W * r, HO = H * r;
    if (i >= (long)N * HO * WO * c8) return;
    const int c = (int)(i % c8) * 8;
    const long m = i / c8;
    const int X = (int)(m % WO), Y = (int)((m / WO) % HO);
    const long n = m / ((long)WO * HO);
    const long sp = (n * H + Y / r) * W + X / r;
    const int sub = (Y % r) * r + X % r;
    f16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = (c + e) * r * r + sub;
        v[e] = src[(long)(ch >> 5) * src_g + sp * 32 + (ch & 31)];
    }
    *(f16x8*)(dst + (long)(c >> 5) * dst_g + m * 32 + (c & 31)) = v;
}

// The launchers of the slab passes: innfer_net_forward and the single-launch entry points (innfer_slab_*, for tests) both go through them, so grid, block and
// argument order under test are the network's.
// map: alpha[C] then shift[C] (device); G: elements of a group, all of them mapped; lo != 0: the (hi, lo) pair form
int launch_input_map(const f16* src, f16* dst, long G, int C, const float* map, int act, hipStream_t s, long lo = 0) {
    const int groups = (C + 31) / 32;
    const long n = G / 8 * groups;
    if (lo) hipLaunchKernelGGL(slab_input_map_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, lo, G, groups, map, C, act);
    else hipLaunchKernelGGL(slab_input_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, G, groups, map, C, act);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int do_input_map(const ConvSlot& cs, const f16* src, f16* dst, long G, hipStream_t s, long lo = 0) {
    return launch_input_map(src, dst, G, cs.C, (const float*)cs.d_map, cs.map_act, s, lo);
}

// PixelShuffle(r) of nf r^2 channels on the h x w grid -> nf channels on r h x r w; lo != 0: once more on the lo twins, `lo` elements behind either slab
int launch_pixel_shuffle(const f16* src, long src_g, f16* dst, long dst_g, int nf, int N, int h, int w, int r, hipStream_t s, long lo = 0) {
    const long nthr = (long)N * h * w * r * r * (nf / 8);
    hipLaunchKernelGGL(slab_pixel_shuffle, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, src, src_g, dst, dst_g, nf, N, h, w, r);
    if (lo) hipLaunchKernelGGL(slab_pixel_shuffle, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, src + lo, src_g, dst + lo, dst_g, nf, N, h, w, r);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// nearest-neighbour f x of `groups` 32-channel groups; lo as above
int launch_upsample_nearest(const f16* src, long src_g, f16* dst, long dst_g, int groups, int N, int h, int w, int f, hipStream_t s, long lo = 0) {
    const long nthr = (long)N * f * f * h * w * 4 * groups;
    hipLaunchKernelGGL(slab_upsample_nearest, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, src, src_g, dst, dst_g, groups, N, h, w, f);
    if (lo) hipLaunchKernelGGL(slab_upsample_nearest, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, src + lo, src_g, dst + lo, dst_g, groups, N, h, w, f);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int do_first(const FirstConvLaunch& F, hipStream_t s) {
    int rc = timed_begin(s);
    if (rc) return rc;
    rc = first_conv_launch(F, s);
    if (rc) return rc;
    rc = debug_after("first_conv", s);
    if (rc) return rc;
    const double px = (double)F.N * F.H * F.W;
    return timed_end(s, 2.0 * 9.0 * F.K * F.Cin * px, px * (F.Cin * (F.in_f32 ? 4.0 : 2.0) + F.K * 2.0 * (F.out2 ? 2 : 1)), 0);
}

// the first conv behind the folded pixel_unshuffle: FLOPs and bytes per LR pixel (3 r^2 input values, K outputs per slab), kind 0 like every first conv
int do_first_unshuffle(const FirstUnshuffleLaunch& F, hipStream_t s) {
    int rc = timed_begin(s);
    if (rc) return rc;
    rc = first_unshuffle_launch(F, s);
    if (rc) return rc;
    rc = debug_after("first_conv_unshuffle", s);
    if (rc) return rc;
    const int cin = F.Cin * F.r * F.r;
    const double px = (double)F.N * ((F.H + F.r - 1) / F.r) * ((F.W + F.r - 1) / F.r);
    return timed_end(s, 2.0 * 9.0 * F.K * cin * px, px * (cin * (F.in_u8 ? 1.0 : F.in_f32 ? 4.0 : 2.0) + F.K * 2.0 * (F.out2 ? 2 : 1)), 0);
}

// in/out point at channel 0 of the tensors; *_g are their group strides (elements).
// lo > 0: fp32-accurate mode, every slab's lo twin `lo` elements behind it
ConvLaunch mk_launch(const ConvSlot& cs, const f16* in, long in_g, void* out, long out_g,
                     int N, int H, int W, int act, long lo) {
    ConvLaunch L{};
    L.in = in; L.in_gstride = in_g; L.C = cs.C;
    L.wpk = (const f16*)(lo ? cs.d_w32 : cs.d_w); L.bias = cs.d_b;
    if (lo) { L.split = 1; L.in_lo = L.out_lo = L.res1_lo = L.res2_lo = lo; }
    L.out = out; L.out_gstride = out_g; L.out_coff = 0; L.K = cs.K;
    L.N = N; L.H = H; L.W = W; L.act = act;
    L.s1 = 1.f; L.s2 = 1.f;
    L.y0 = 0; L.y1 = H;
    L.out_mode = OUT_SLAB;
    L.conv1x1 = cs.ksize == 1;
    L.rowp = (!lo && cs.rowp) ? 1 : 0;          // (the split panels keep the lane-contiguous order)
    return L;
}

// SRVGGNetCompact (kind 2): first conv -> slab A; num_conv convs ping-pong A <-> B, ONE launch each with the activation (act 8) in its epilogue; the last conv -> the tail
// slab; shuffle_add_launch writes PixelShuffle(scale)(tail) + nearest_upsample(input) to d_out.  Whole-frame launches (band_rows is not used here).
int compact_forward(innfer_net* net, const void* d_in, int in_dtype, void* d_out, int out_dtype, int N, int H, int W, char* ws, const Carve& cv, hipStream_t s) {
    if (in_dtype == INNFER_F32 || net->fp32) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SRVGGNetCompact is built for the fp16 mode only: fp16 or uint8 input");
    if (net->outm || net->final_act) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SRVGGNetCompact has no outm / final activation");
    if (in_dtype == INNFER_U8 && !net->u8_round16) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SRVGGNetCompact is built for the fp16 mode only (innfer_net_set_u8_io fp16_mode = 1)");
    for (auto& c : net->convs)
        if (c.slope_ok && !c.d_slope) return set_error(INNFER_ERR_INVALID, "forward: the activation slopes of '%s' were never set (innfer_net_set_conv_slope)", c.key.c_str());
    const long G = (long)N * H * W * 32;
    f16* ab[2] = {(f16*)(ws + cv.slab[0]), (f16*)(ws + cv.slab[1])};
    f16* tail = (f16*)(ws + cv.hr);
    int ci = 0;
    {
        const ConvSlot& c0 = net->convs[ci++];
        FirstConvLaunch F{};
        F.in = d_in; F.in_f32 = 0; F.Cin = c0.C; F.w = (const float*)c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = 1;
        F.out = ab[0]; F.out_gstride = G;
        F.K = net->nf; F.N = N; F.H = H; F.W = W; F.act = 8; F.slope = c0.d_slope;
        if (int rc = do_first(F, s)) return rc;
    }
    int cur = 0;
    for (int i = 0; i < net->nb; ++i) {
        const ConvSlot& cs = net->convs[ci++];
        ConvLaunch L = mk_launch(cs, ab[cur], G, ab[cur ^ 1], G, N, H, W, 8, 0);
        L.slope = cs.d_slope;
        if (int rc = do_conv(L, s)) return rc;
        cur ^= 1;
    }
    const ConvSlot& cl = net->convs[ci++];
    {
        ConvLaunch L = mk_launch(cl, ab[cur], G, tail, G, N, H, W, 0, 0);
        L.K = cl.Kp;
        if (int rc = do_conv(L, s)) return rc;
    }
    ShuffleAddLaunch T{};
    T.slab = tail; T.gstride = G;
    T.base = d_in; T.base_u8 = in_dtype == INNFER_U8; T.base_norm = net->u8_normalize;
    T.out = d_out; T.out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0; T.out_denorm = net->u8_normalize;
    T.C = net->out_nc; T.s = net->scale; T.N = N; T.H = H; T.W = W;
    if (int rc = timed_begin(s)) return rc;
    if (int rc = shuffle_add_launch(T, s)) return rc;
    if (int rc = debug_after("shuffle_add", s)) return rc;
    const double px = (double)N * H * W, k = (double)cl.K;
    // launch kind 6000: the tail -- one add per output value; bytes: the K valid slab channels and the input in, the result out
    return timed_end(s, px * k, px * (k * 2.0 + net->in_nc * (T.base_u8 ? 1.0 : 2.0) + k * (T.out_mode == 2 ? 1.0 : T.out_mode == 1 ? 4.0 : 2.0)), 6000);
}

// dst = SiLU(src) over n8 runs of eight fp16 values: v * sigmoid(v) in fp32 on the stored value, one rounding (SPAN's block_6 keeps its first conv's result raw for the
// concat, so that one activation is a pass of its own)
__global__ void slab_silu(const f16* src, f16* dst, long n8) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const f16x8 x = *(const f16x8*)(src + i * 8);
    f16x8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float v = (float)x[e]; y[e] = (f16)(v * fast_sigmoid(v)); }
    *(f16x8*)(dst + i * 8) = y;
}

// SPAN (kind 3).  cat = the concat slab, four ranges of nf channels (whole 32-channel groups: torch.cat is a pointer): [f0 | conv_2(b6) | b1 | b5_2].
//   conv_1 (input map when norm) -> cat[0]; block_i: c1_r act 9, c2_r act 9, c3_r act 10 with res1 = the block's input, rotating through three slabs (block_1 writes its
//   result to cat[2]); block_6's c1_r runs without activation into cat[3] and slab_silu makes its activated copy; conv_2 -> cat[1]; conv_cat (1x1, 4 nf -> nf);
//   upsampler.0 -> tail slab; shuffle_add_launch without a base = PixelShuffle(scale) to d_out.  24 launches.
int span_forward(innfer_net* net, const void* d_in, int in_dtype, void* d_out, int out_dtype, int N, int H, int W, char* ws, const Carve& cv, hipStream_t s) {
    if (in_dtype == INNFER_F32 || net->fp32) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SPAN is built for the fp16 mode only: fp16 or uint8 input");
    if (net->outm || net->final_act) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SPAN has no outm / final activation");
    if (in_dtype == INNFER_U8 && !net->u8_round16) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SPAN is built for the fp16 mode only (innfer_net_set_u8_io fp16_mode = 1)");
    const long G = (long)N * H * W * 32;
    const int g = net->nf / 32;
    f16* cat = (f16*)(ws + cv.fea);
    f16* cat_r[4] = {cat, cat + (long)g * G, cat + 2L * g * G, cat + 3L * g * G};
    f16* rot[3] = {(f16*)(ws + cv.slab[0]), (f16*)(ws + cv.slab[1]), (f16*)(ws + cv.slab[2])};
    f16* tail = (f16*)(ws + cv.hr);
    int ci = 0;
    {
        const ConvSlot& c0 = net->convs[ci++];
        FirstConvLaunch F{};
        F.in = d_in; F.in_f32 = 0; F.Cin = c0.C; F.w = (const float*)c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = 1;
        F.out = cat_r[0]; F.out_gstride = G;
        F.K = net->nf; F.N = N; F.H = H; F.W = W; F.act = 0;
        F.in_map = net->span_norm ? c0.d_map : nullptr;
        if (int rc = do_first(F, s)) return rc;
    }
    const f16* x = cat_r[0];             // the current block's input
    for (int b = 1; b <= 6; ++b) {
        f16* t1 = rot[0] != x ? rot[0] : rot[1];           // two of the three slabs that do not hold x
        f16* t2 = rot[2] != x && rot[2] != t1 ? rot[2] : rot[1];
        f16* dst = b == 1 ? cat_r[2] : t1;                 // (c3_r reads t2 and x: t1 is free again once c2_r has read it)
        const ConvSlot& c1 = net->convs[ci++];
        const ConvSlot& c2 = net->convs[ci++];
        const ConvSlot& c3 = net->convs[ci++];
        if (b < 6) {
            ConvLaunch L1 = mk_launch(c1, x, G, t1, G, N, H, W, 9, 0);
            if (int rc = do_conv(L1, s)) return rc;
        } else {
            ConvLaunch L1 = mk_launch(c1, x, G, cat_r[3], G, N, H, W, 0, 0);
            if (int rc = do_conv(L1, s)) return rc;
            if (int rc = timed_begin(s)) return rc;
            const long n8 = (long)g * G / 8;
            hipLaunchKernelGGL(slab_silu, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, (const f16*)cat_r[3], t1, n8);
            INNFER_HIP(hipGetLastError());
            if (int rc = debug_after("slab_silu", s)) return rc;
            // launch kind 6001: the SiLU pass -- bytes: nf channels in and out
            if (int rc = timed_end(s, (double)n8 * 8, (double)n8 * 8 * 4.0, 6001)) return rc;
        }
        ConvLaunch L2 = mk_launch(c2, t1, G, t2, G, N, H, W, 9, 0);
        if (int rc = do_conv(L2, s)) return rc;
        ConvLaunch L3 = mk_launch(c3, t2, G, dst, G, N, H, W, 10, 0);
        L3.res1 = x; L3.res1_gstride = G;
        if (int rc = do_conv(L3, s)) return rc;
        x = dst;
    }
    {
        const ConvSlot& c2 = net->convs[ci++];
        ConvLaunch L = mk_launch(c2, x, G, cat_r[1], G, N, H, W, 0, 0);
        if (int rc = do_conv(L, s)) return rc;
    }
    f16* fused = rot[0] == x ? rot[1] : rot[0];
    {
        const ConvSlot& cc = net->convs[ci++];
        ConvLaunch L = mk_launch(cc, cat, G, fused, G, N, H, W, 0, 0);
        if (int rc = do_conv(L, s)) return rc;
    }
    const ConvSlot& cl = net->convs[ci++];
    {
        ConvLaunch L = mk_launch(cl, fused, G, tail, G, N, H, W, 0, 0);
        L.K = cl.Kp;
        if (int rc = do_conv(L, s)) return rc;
    }
    ShuffleAddLaunch T{};
    T.slab = tail; T.gstride = G;
    T.base = nullptr;
    T.out = d_out; T.out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0; T.out_denorm = net->u8_normalize;
    T.C = net->out_nc; T.s = net->scale; T.N = N; T.H = H; T.W = W;
    if (int rc = timed_begin(s)) return rc;
    if (int rc = shuffle_add_launch(T, s)) return rc;
    if (int rc = debug_after("shuffle (SPAN tail)", s)) return rc;
    const double px = (double)N * H * W, k = (double)cl.K;
    return timed_end(s, 0.0, px * (k * 2.0 + k * (T.out_mode == 2 ? 1.0 : T.out_mode == 1 ? 4.0 : 2.0)), 6000);
}

// RealPLKSR (kind 4).  Per block, on x (two groups): channel_mixer.0 as two act-11 launches -> M (four groups); channel_mixer.2 -> groups 0 and 2 of the three-group
// buffer [U0 | T0 | U1] (output group stride 2 G); plk_conv U0 -> T0 (its channels 16 .. 31 copied), so [T0 | U1] at stride G is lk's result; the EA gate (act 5 with
// res1 = its own input) -> M[0, 1]; refine (1x1) -> M[2, 3]; GroupNorm statistics, finalize, and x = fp16(alpha u + shift + x) in place.  9 launches (8 without EA);
// the tail is SRVGGNetCompact's: the last conv, then shuffle_add with the input as base.  9 n_blocks + 3 launches at most.
static int plksr_pass(hipStream_t s, const char* what, double flops, double bytes, int kind, const std::function<int()>& launch) {
    if (int rc = timed_begin(s)) return rc;
    if (int rc = launch()) return rc;
    if (int rc = debug_after(what, s)) return rc;
    return timed_end(s, flops, bytes, kind);
}

int plksr_forward(innfer_net* net, const void* d_in, int in_dtype, void* d_out, int out_dtype, int N, int H, int W, char* ws, const Carve& cv, hipStream_t s) {
    if (in_dtype == INNFER_F32 || net->fp32) return set_error(INNFER_ERR_UNSUPPORTED, "forward: RealPLKSR is built for the fp16 mode only: fp16 or uint8 input");
    if (net->outm || net->final_act) return set_error(INNFER_ERR_UNSUPPORTED, "forward: RealPLKSR has no outm / final activation");
    if (in_dtype == INNFER_U8 && !net->u8_round16) return set_error(INNFER_ERR_UNSUPPORTED, "forward: RealPLKSR is built for the fp16 mode only (innfer_net_set_u8_io fp16_mode = 1)");
    for (auto& c : net->convs)
        if (c.gn_ok && !c.d_gn) return set_error(INNFER_ERR_INVALID, "forward: the GroupNorm parameters behind '%s' were never set (innfer_net_set_group_norm)", c.key.c_str());
    const long HW = (long)H * W, G = (long)N * HW * 32;
    const double px = (double)N * HW;
    f16* x = (f16*)(ws + cv.fea);
    f16* M = (f16*)(ws + cv.slab[0]);
    f16* U = (f16*)(ws + cv.slab[1]);
    f16* tail = (f16*)(ws + cv.hr);
    float* work = (float*)(ws + cv.tmp);
    int ci = 0;
    {
        const ConvSlot& c0 = net->convs[ci++];
        FirstConvLaunch F{};
        F.in = d_in; F.in_f32 = 0; F.Cin = c0.C; F.w = (const float*)c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = 1;
        F.out = x; F.out_gstride = G;
        F.K = net->nf; F.N = N; F.H = H; F.W = W; F.act = 0;
        if (int rc = do_first(F, s)) return rc;
    }
    for (int b = 0; b < net->nb; ++b) {
        const ConvSlot& ca = net->convs[ci++];
        const ConvSlot& cb = net->convs[ci++];
        const ConvSlot& c2 = net->convs[ci++];
        const ConvSlot& lk = net->convs[ci++];
        const ConvSlot* ea = net->plk_ea ? &net->convs[ci++] : nullptr;
        const ConvSlot& rf = net->convs[ci++];
        ConvLaunch La = mk_launch(ca, x, G, M, G, N, H, W, 11, 0);
        if (int rc = do_conv(La, s)) return rc;
        ConvLaunch Lb = mk_launch(cb, x, G, M + 2 * G, G, N, H, W, 11, 0);
        if (int rc = do_conv(Lb, s)) return rc;
        ConvLaunch L2 = mk_launch(c2, M, G, U, 2 * G, N, H, W, 0, 0);
        if (int rc = do_conv(L2, s)) return rc;
        PlkLaunch P{U, U + G, (const f16*)lk.d_w, lk.d_b, lk.ksize, N, H, W};
        // launch kind 7000: the partial large-kernel conv -- bytes: one group in, one out, the panel
        if (int rc = plksr_pass(s, "plk_conv", 2.0 * lk.ksize * lk.ksize * 256.0 * px, px * 128.0 + lk.ksize * lk.ksize * 512.0, 7000, [&] { return plk_conv_launch(P, s); })) return rc;
        const f16* v = U + G;
        if (ea) {
            ConvLaunch Le = mk_launch(*ea, U + G, G, M, G, N, H, W, 5, 0);
            Le.res1 = U + G; Le.res1_gstride = G;
            if (int rc = do_conv(Le, s)) return rc;
            v = M;
        }
        f16* u = M + 2 * G;
        ConvLaunch Lr = mk_launch(rf, v, G, u, G, N, H, W, 0, 0);
        if (int rc = do_conv(Lr, s)) return rc;
        // launch kinds 7001 .. 7003: the GroupNorm statistics, their merge, and norm + skip
        if (int rc = plksr_pass(s, "gn_stats", 3.0 * 64 * px, px * 128.0, 7001, [&] { return gn_stats_launch(u, G, N, HW, work, s); })) return rc;
        if (int rc = plksr_pass(s, "gn_finalize", 0.0, 0.0, 7002, [&] { return gn_finalize_launch(N, HW, net->plk_groups, rf.d_gn, rf.d_gn + 64, 1e-5f, work, s); })) return rc;
        if (int rc = plksr_pass(s, "gn_apply", 2.0 * 64 * px, px * 384.0, 7003, [&] { return gn_apply_launch(u, G, x, G, x, G, N, HW, work, s); })) return rc;
    }
    const ConvSlot& cl = net->convs[ci++];
    {
        ConvLaunch L = mk_launch(cl, x, G, tail, G, N, H, W, 0, 0);
        L.K = cl.Kp;
        if (int rc = do_conv(L, s)) return rc;
    }
    ShuffleAddLaunch T{};
    T.slab = tail; T.gstride = G;
    T.base = d_in; T.base_u8 = in_dtype == INNFER_U8; T.base_norm = net->u8_normalize;
    T.out = d_out; T.out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0; T.out_denorm = net->u8_normalize;
    T.C = net->out_nc; T.s = net->scale; T.N = N; T.H = H; T.W = W;
    const double k = (double)cl.K;
    return plksr_pass(s, "shuffle_add", px * k, px * (k * 2.0 + net->in_nc * (T.base_u8 ? 1.0 : 2.0) + k * (T.out_mode == 2 ? 1.0 : T.out_mode == 1 ? 4.0 : 2.0)), 6000, [&] { return shuffle_add_launch(T, s); });
}

// dst[o][y][x] = src[o][ry][rx] over `outer` planes of `inner`-byte pixels: a window copy between two sizes.  dst larger: F.pad(.., (0, pw, 0, ph), 'reflect') -- row y >= sh
// reads row 2 (sh - 1) - y; dst smaller: the crop to its top-left dh x dw.  Planar tensors: outer = N C, inner = the element; uint8 HWC images: outer = N, inner = C.
__global__ void rect_copy(const uint8_t* src, uint8_t* dst, long outer, int sh, int sw, int dh, int dw, int inner) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= outer * dh * dw) return;
    const int x = (int)(i % dw), y = (int)((i / dw) % dh);
    const long o = i / ((long)dw * dh);
    const int ry = y < sh ? y : 2 * (sh - 1) - y, rx = x < sw ? x : 2 * (sw - 1) - x;
    const uint8_t* q = src + ((o * sh + ry) * sw + rx) * inner;
    for (int b = 0; b < inner; ++b) dst[i * inner + b] = q[b];
}

// SwinIR (kind 5) on the padded grid Hp x Wp (multiples of 8).  [pad]; conv_first (the input map x - mean its prologue) in C_pad / 64 launches -> f0; r = LN(f0);
// per residual group: per block  u = LN(t); qkv (ceil(3 nH / 2) launches of two head groups); the window attention; proj + shortcut (C_pad / 64 launches, res1 = the
// block's input: the group's input r for its first block, else t in place); u = LN(t); fc1 with GELU (act 12; hidden_pad / 64 launches); fc2 + shortcut (in place);
// then r' = conv(t) + r into the other r buffer.  t = LN(r); F = conv_after_body(t) + f0; the tail; [crop].
static int swinir_forward(innfer_net* net, const void* d_in, int in_dtype, void* d_out, int out_dtype, int N, int H, int W, char* ws, hipStream_t s) {
    if (in_dtype == INNFER_F32 || net->fp32) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SwinIR is built for the fp16 mode only: fp16 or uint8 input");
    if (net->outm || net->final_act) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SwinIR has no outm / final activation");
    if (in_dtype == INNFER_U8 && !net->u8_round16) return set_error(INNFER_ERR_UNSUPPORTED, "forward: SwinIR is built for the fp16 mode only (innfer_net_set_u8_io fp16_mode = 1)");
    for (size_t i = 0; i < net->sw_ln.size(); ++i)
        if (!net->sw_ln[i]) return set_error(INNFER_ERR_INVALID, "forward: the parameters of LayerNorm %zu were never set (innfer_net_set_layer_norm)", i);
    for (size_t i = 0; i < net->sw_relb.size(); ++i)
        if (!net->sw_relb[i] && !(net->kind == 8 && net->dat_aca[i])) return set_error(INNFER_ERR_INVALID, "forward: the relative position bias of block %zu was never set (innfer_net_set_attn_bias)", i);
    for (size_t i = 0; i < net->sw_tau.size(); ++i)
        if (!net->sw_tau[i]) return set_error(INNFER_ERR_INVALID, "forward: the attention scale of block %zu was never set (innfer_net_set_attn_scale)", i);
    const SwinCarve cv = swin_carve(net, N, H, W);
    const int Hp = cv.Hp, Wp = cv.Wp, sc = net->scale, cp = net->sw_cp, nh = net->sw_nh;
    if (Hp - H >= H || Wp - W >= W) return set_error(INNFER_ERR_INVALID, "forward: %d x %d cannot be reflect-padded to %d x %d (the pad must be smaller than the side)", H, W, Hp, Wp);
    const bool padded = Hp != H || Wp != W;
    const long npx = (long)N * Hp * Wp, G = npx * 32;
    const double px = (double)npx;
    const int omode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0;
    auto window = [&](const char* what, const void* src, void* dst, long outer, int sh, int sw, int dh, int dw, int inner, int kind) {
        const long n = outer * dh * dw;
        return plksr_pass(s, what, 0.0, 2.0 * n * inner, kind, [&] {
            hipLaunchKernelGGL(rect_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t*)src, (uint8_t*)dst, outer, sh, sw, dh, dw, inner);
            INNFER_HIP(hipGetLastError());
            return (int)INNFER_OK;
        });
    };
    auto norm = [&](int idx, const f16* in, f16* out) {
        // launch kind 8000: LayerNorm -- bytes: C_pad channels in and out
        return plksr_pass(s, "layer_norm", 8.0 * net->sw_c * px, px * cp * 4.0, 8000,
                          [&] { return layer_norm_launch(in, G, out, G, npx, net->sw_c, cp, net->sw_ln[idx], net->sw_ln[idx] + cp, 1e-5f, s); });
    };
    // a conv cut into 64-output launches: slice p writes channel groups 2 p, 2 p + 1 of `out` (and adds the same groups of `res`)
    int ci = 0;
    auto sliced = [&](int nslices, const f16* in, f16* out, int act, const f16* res) {
        for (int p = 0; p < nslices; ++p) {
            const ConvSlot& cs = net->convs[ci++];
            ConvLaunch L = mk_launch(cs, in, G, out + 2L * p * G, G, N, Hp, Wp, act, 0);
            if (res) { L.res1 = res + 2L * p * G; L.res1_gstride = G; L.s1 = 1.f; }
            if (int rc = do_conv(L, s)) return rc;
        }
        return (int)INNFER_OK;
    };
    auto resi = [&](const f16* in, f16* out, const f16* res) {
        if (!net->sw_conv3) return sliced(cp / 64, in, out, 0, res);
        f16 *a = (f16*)(ws + cv.c4[0]), *b = (f16*)(ws + cv.c4[1]);
        if (int rc = sliced(net->sw_c4p / 64, in, a, 1, nullptr)) return rc;
        if (int rc = sliced(net->sw_c4p / 64, a, b, 1, nullptr)) return rc;
        return sliced(cp / 64, b, out, 0, res);
    };
    const void* xin = d_in;
    if (padded) {
        xin = ws + cv.xin;
        // launch kind 8002: the reflect pad of the input (8003: the crop of the result)
        if (int rc = in_dtype == INNFER_U8 ? window("reflect pad", d_in, ws + cv.xin, N, H, W, Hp, Wp, net->in_nc, 8002)
                                           : window("reflect pad", d_in, ws + cv.xin, (long)N * net->in_nc, H, W, Hp, Wp, 2, 8002)) return rc;
    }
    f16* f0 = (f16*)(ws + cv.f0);
    f16* r[2] = {(f16*)(ws + cv.r[0]), (f16*)(ws + cv.r[1])};
    f16* t = (f16*)(ws + cv.t);
    f16* u = (f16*)(ws + cv.u);
    f16* qkv = (f16*)(ws + cv.qkv);
    f16* att = (f16*)(ws + cv.att);
    f16* hid = (f16*)(ws + cv.hid);
    const float* in_map = net->convs[0].d_map;
    for (int p = 0; p < cp / 64; ++p) {
        const ConvSlot& c0 = net->convs[ci++];
        FirstConvLaunch F{};
        F.in = xin; F.in_f32 = 0; F.Cin = c0.C; F.w = (const float*)c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = 1;
        F.out = f0 + 2L * p * G; F.out_gstride = G;
        F.K = 64; F.N = N; F.H = Hp; F.W = Wp; F.act = 0;
        F.in_map = in_map;
        if (int rc = do_first(F, s)) return rc;
    }
    int cur = 0, blk = 0;
    if (int rc = norm(0, f0, r[0])) return rc;
    if (net->kind == 6) {
        // HAT: per HAB  u = LN(t); z = cab.2(GELU(cab.0(u))) (act 13: one launch, then C_pad / 64); the channel sums of z and the squeeze / excite vector y; qkv; the 16 x 16
        // window attention (shift 8 for odd j); proj + shortcut -> t; t += conv_scale y z; u = LN(t); fc1 with GELU; fc2 + shortcut.  Per residual group, behind its HABs,
        // the OCAB: u = LN(t); qkv; the overlapping attention (24 x 24 keys); proj + shortcut; u = LN(t); fc1; fc2 + shortcut.  Then r' = conv(t) + r.
        for (size_t i = 0; i < net->hat_ca.size(); ++i)
            if (!net->hat_ca[i]) return set_error(INNFER_ERR_INVALID, "forward: the channel attention of block %zu was never set (innfer_net_set_chan_attn)", i);
        f16* zc = (f16*)(ws + cv.zc);
        f16* z = (f16*)(ws + cv.z);
        float* y = (float*)(ws + cv.y);
        float* pool = (float*)(ws + cv.pool);
        const long HWp = (long)Hp * Wp;
        const int C = net->sw_c, sq = net->hat_sq;
        int ln = 1, tb = 0;
        auto attn = [&](int kw, int shift) {
            // launch kind 8001: the window attention -- bytes: q, k, v in, o out (32-channel head groups), the bias table
            const double nk = (double)kw * kw;
            return plksr_pass(s, kw == 16 ? "window_attention16" : "overlap_attention", 4.0 * nk * 32 * nh * px, px * nh * 256.0 + nh * 1024.0 * nk, 8001,
                              [&] { return win_attn16_launch(qkv, G, att, G, net->sw_relb[tb], N, Hp, Wp, nh, net->sw_d, shift, kw, s); });
        };
        for (size_t i = 0; i < net->sw_depths.size(); ++i) {
            for (int j = 0; j < net->sw_depths[i]; ++j, ++blk, ++tb) {
                const f16* x = j == 0 ? r[cur] : t;
                if (int rc = norm(ln++, x, u)) return rc;
                if (int rc = sliced(1, u, zc, 13, nullptr)) return rc;
                if (int rc = sliced(cp / 64, zc, z, 0, nullptr)) return rc;
                const float* ca = net->hat_ca[blk];
                // launch kinds 8005 / 8006 / 8007: the channel sums, the squeeze / excite vector, the scale-add pass
                if (int rc = plksr_pass(s, "chan_attn_pool", px * cp, px * cp * 2.0, 8005, [&] { return ca_pool_launch(z, G, N, HWp, cp, pool, s); })) return rc;
                if (int rc = plksr_pass(s, "chan_attn_excite", 4.0 * C * sq * N, 4.0 * (double)ca_work_floats(N, HWp, cp), 8006, [&] {
                        return ca_excite_launch(pool, N, HWp, C, cp, sq, ca, ca + (long)sq * C, ca + (long)sq * C + sq, ca + 2L * sq * C + sq, y, nullptr, s); })) return rc;
                if (int rc = sliced((3 * nh + 1) / 2, u, qkv, 0, nullptr)) return rc;
                if (int rc = attn(16, (j & 1) ? 8 : 0)) return rc;
                if (int rc = sliced(cp / 64, att, t, 0, x)) return rc;
                if (int rc = plksr_pass(s, "chan_attn_scale_add", 2.0 * px * cp, px * cp * 6.0, 8007, [&] { return ca_scale_add_launch(t, G, z, G, y, net->hat_scale, N, HWp, cp, s); })) return rc;
                if (int rc = norm(ln++, t, u)) return rc;
                if (int rc = sliced(net->sw_hp / 64, u, hid, 12, nullptr)) return rc;
                if (int rc = sliced(cp / 64, hid, t, 0, t)) return rc;
            }
            if (int rc = norm(ln++, t, u)) return rc;
            if (int rc = sliced((3 * nh + 1) / 2, u, qkv, 0, nullptr)) return rc;
            if (int rc = attn(24, 0)) return rc;
            ++tb;
            if (int rc = sliced(cp / 64, att, t, 0, t)) return rc;
            if (int rc = norm(ln++, t, u)) return rc;
            if (int rc = sliced(net->sw_hp / 64, u, hid, 12, nullptr)) return rc;
            if (int rc = sliced(cp / 64, hid, t, 0, t)) return rc;
            if (int rc = resi(t, r[cur ^ 1], r[cur])) return rc;
            cur ^= 1;
        }
    } else if (net->kind == 9) {
        // DRCT: r[cur] is the dense slab D = x | x1 | x2 | x3 | x4 of the current group (x in its own gx groups, x_k in group gx + k - 1).  Per block k = 0 .. 4:
        // u = LN(D[: dim_k]) (the holed form); qkv into the head-padded slab (a head owns G = ceil(d / 32) groups); the 16 x 16 attention (win_attn16 for d <= 32, the wide
        // kernel above; shift 8 for k = 1, 3); proj + shortcut from D -> t; u = LN(t); fc1 with GELU; fc2 + shortcut in place; then adjust: k < 4 ONE 64-output launch with
        // LeakyReLU(0.2) that writes x_{k+1} into group gx + k of D and ZEROS into group gx + k + 1 (its rows 32 .. 63 are zero), k = 4 the S1 launches 0.2 * . + x into the
        // other dense slab -- the next group's x.  No group is read by a matrix product before it is written: a product reads 32 ng_k channels, never the rounded-up width;
        // the rounded-up groups a LayerNorm or a shortcut touches hold the zeros of the launch before (or the pad group of x), and the LayerNorm selects, never multiplies.
        const DrctDims dd = drct_dims(net);
        const int C = net->sw_c;
        int ln = 1;
        auto hnorm = [&](int idx, const f16* in, f16* out, int k) {
            return plksr_pass(s, "layer_norm_holed", 8.0 * (C + 32 * k) * px, px * dd.lp[k] * 4.0, 8000, [&] {
                return layer_norm_holed_launch(in, G, out, G, npx, C, dd.cpk[k], dd.lp[k], net->sw_ln[idx], net->sw_ln[idx] + dd.lp[k], 1e-5f, s); });
        };
        for (int i = 0; i < net->dr_r; ++i) {
            f16 *D = r[cur], *Dn = r[cur ^ 1];
            for (int k = 0; k < 5; ++k, ++blk) {
                const int nhb = net->dr_nh[blk], d = (C + 32 * k) / nhb, hg = drct_head_groups(net, (size_t)blk), S = dd.lp[k] / 64, SH = (net->dr_hid[blk] + 63) / 64;
                const int shift = (k & 1) ? 8 : 0;
                if (int rc = hnorm(ln++, D, u, k)) return rc;
                if (int rc = sliced((3 * hg + 1) / 2, u, qkv, 0, nullptr)) return rc;
                // launch kind 8001: the window attention -- bytes: q, k, v in, o out (the head groups), the bias table
                if (int rc = plksr_pass(s, d <= 32 ? "window_attention16" : "window_attention16_wide", 4.0 * 256 * (C + 32 * k) * px, px * hg * 256.0 + nhb * 262144.0, 8001, [&] {
                        return d <= 32 ? win_attn16_launch(qkv, G, att, G, net->sw_relb[blk], N, Hp, Wp, nhb, d, shift, 16, s)
                                       : win_attn16_wide_launch(qkv, G, att, G, net->sw_relb[blk], N, Hp, Wp, nhb, d, shift, s); })) return rc;
                if (int rc = sliced(S, att, t, 0, D)) return rc;
                if (int rc = hnorm(ln++, t, u, k)) return rc;
                if (int rc = sliced(SH, u, hid, 12, nullptr)) return rc;
                if (int rc = sliced(S, hid, t, 0, t)) return rc;
                if (k < 4) {
                    if (int rc = sliced(1, t, D + (long)dd.ng[k] * G, 1, nullptr)) return rc;
                } else {
                    for (int p = 0; p < cp / 64; ++p) {
                        const ConvSlot& cs = net->convs[ci++];
                        ConvLaunch L = mk_launch(cs, t, G, Dn + 2L * p * G, G, N, Hp, Wp, 0, 0);
                        L.res1 = D + 2L * p * G; L.res1_gstride = G; L.s1 = 0.2f;          // 0.2 * x5 + x
                        if (int rc = do_conv(L, s)) return rc;
                    }
                }
            }
            cur ^= 1;
        }
    } else if (net->kind == 8) {
        // DAT on H x W itself (Hp = H, Wp = W: no pad, no crop).  Per block  u = LN(t); qkv; the attention into `att` -- even index in its group: rectangular windows (one
        // launch); odd: across channels (Gram, merge + softmax, apply) --; c = GELU(dwconv(v)) on the v groups of the qkv slab (BatchNorm folded); the pool over Y and the
        // GELU excite; the interaction mix in place on `att` ((X, Y) = (att, c) | (c, att)); proj + shortcut; u = LN(t); fc1 with GELU into [x1 | x2]; LN(x2); x2 = x1 *
        // dwconv(LN(x2)); fc2 from x2 + shortcut.  9 + SQ + 2 S1 + SF launches (11 + ... for the channel form), SF = 2 h1p / 64.  Then r' = conv(t) + r.
        for (size_t i = 0; i < net->dat_blk.size(); ++i)
            if (!net->dat_blk[i]) return set_error(INNFER_ERR_INVALID, "forward: the parameters of block %zu were never set (innfer_net_set_dat_block)", i);
        const DatOff o = dat_offsets(net);
        const long HW = (long)H * W;
        const int chp = 32 * nh, hc = net->sw_c / 8, hs = net->sw_c / 16, half = net->sw_hid / 2, h1p = net->dat_h1p, T = net->dat_s0 * net->dat_s1;
        f16* cb = (f16*)(ws + cv.z);
        f16* sg = (f16*)(ws + cv.zc);
        float* y = (float*)(ws + cv.y);
        float* pool = (float*)(ws + cv.pool);
        float* gram = (float*)(ws + cv.gram);
        float* amat = (float*)(ws + cv.amat);
        f16* x1 = hid;
        f16* x2 = hid + (long)(h1p / 32) * G;
        const f16* vg = qkv + 2L * nh * G;
        for (size_t i = 0; i < net->sw_depths.size(); ++i) {
            for (int j = 0; j < net->sw_depths[i]; ++j, ++blk) {
                const float* P = net->dat_blk[blk];
                const bool aca = net->dat_aca[blk] != 0;
                const f16* x = j == 0 ? r[cur] : t;
                if (int rc = norm(1 + 2 * blk, x, u)) return rc;
                if (int rc = sliced((3 * nh + 1) / 2, u, qkv, 0, nullptr)) return rc;
                // launch kinds 8001 the window attention; 8010 / 8011 / 8012 the channel attention's Gram, merge + softmax, apply; 8013 the depthwise conv; 8005 / 8006 the
                // pool and the excite; 8014 the interaction mix; 8000 LayerNorm
                if (!aca) {
                    if (int rc = plksr_pass(s, "window_attention_rect", 4.0 * T * 32 * nh * px, px * nh * 256.0 + nh * 4.0 * T * T, 8001, [&] {
                            return win_attn_rect_launch(qkv, G, att, G, net->sw_relb[blk], N, H, W, nh, net->sw_d, net->dat_s0, net->dat_s1, net->dat_shift[blk], s); })) return rc;
                } else {
                    if (int rc = plksr_pass(s, "channel_attention_gram", 2.0 * 1088 * nh * px, 128.0 * nh * px, 8010, [&] { return csa_gram_launch(qkv, G, N, HW, nh, net->sw_d, gram, s); })) return rc;
                    if (int rc = plksr_pass(s, "channel_attention_softmax", 0.0, 4.0 * (double)csa_work_floats(N, HW, nh), 8011, [&] {
                            return csa_softmax_launch(gram, N, HW, nh, net->sw_d, P + o.temp, amat, nullptr, s); })) return rc;
                    if (int rc = plksr_pass(s, "channel_attention_apply", 2.0 * 1024 * nh * px, 128.0 * nh * px, 8012, [&] { return csa_apply_launch(qkv, G, att, G, amat, N, HW, nh, net->sw_d, s); })) return rc;
                }
                if (int rc = plksr_pass(s, "dwconv_gelu", 18.0 * chp * px, 4.0 * chp * px, 8013, [&] {
                        return dwconv3x3_launch(vg, G, nullptr, 0, cb, G, N, H, W, chp, chp, P + o.dw_t, P + o.dw_b, 1, s); })) return rc;
                const f16* X = aca ? cb : att;
                const f16* Y = aca ? att : cb;
                if (int rc = plksr_pass(s, "chan_attn_pool", px * chp, px * chp * 2.0, 8005, [&] { return ca_pool_launch(Y, G, N, HW, chp, pool, s); })) return rc;
                if (int rc = plksr_pass(s, "chan_attn_excite_gelu", 4.0 * chp * hc * N, 4.0 * (double)ca_work_floats(N, HW, chp), 8006, [&] {
                        return ca_excite_gelu_launch(pool, N, HW, chp, chp, hc, P + o.ci_w1, P + o.ci_b1, P + o.ci_w2, P + o.ci_b2, y, nullptr, s); })) return rc;
                if (int rc = plksr_pass(s, "aim_mix", (2.0 * chp * hs + 3.0 * chp) * px, 6.0 * chp * px, 8014, [&] {
                        return aim_mix_launch(X, G, Y, G, att, G, y, N, HW, chp, chp, hs, P + o.si_w1, P + o.si_b1, P + o.si_w2, net->dat_sib2[blk], s); })) return rc;
                if (int rc = sliced(cp / 64, att, t, 0, x)) return rc;
                if (int rc = norm(2 + 2 * blk, t, u)) return rc;
                if (int rc = sliced(2 * h1p / 64, u, hid, 12, nullptr)) return rc;
                if (int rc = plksr_pass(s, "layer_norm_wide", 8.0 * half * px, px * h1p * 4.0, 8000, [&] {
                        return layer_norm_wide_launch(x2, G, sg, G, npx, half, h1p, P + o.sg_g, P + o.sg_b, 1e-5f, s); })) return rc;
                if (int rc = plksr_pass(s, "dwconv_gate", 18.0 * half * px, 6.0 * h1p * px, 8013, [&] {
                        return dwconv3x3_launch(sg, G, x1, G, x2, G, N, H, W, half, h1p, P + o.sg_t, P + o.sg_cb, 2, s); })) return rc;
                if (int rc = sliced(cp / 64, x2, t, 0, t)) return rc;
            }
            if (int rc = resi(t, r[cur ^ 1], r[cur])) return rc;
            cur ^= 1;
        }
    } else if (net->kind == 7) {
        // Swin2SR: per block  qkv from the token stream itself; the cosine window attention; u = proj (no shortcut); t = x + LN(u) (one launch; x the group's input r for
        // its first block, else t in place); fc1 with GELU from t; u = fc2; t = t + LN(u).  The same launch count as SwinIR's block: 3 + SQ + 2 S1 + SH.
        auto norm_add = [&](int idx, const f16* in, const f16* res, f16* out) {
            // launch kind 8008: LayerNorm + residual -- bytes: C_pad channels of the branch and of the stream in, the stream out
            return plksr_pass(s, "layer_norm_add", 9.0 * net->sw_c * px, px * cp * 6.0, 8008,
                              [&] { return layer_norm_add_launch(in, G, res, G, out, G, npx, net->sw_c, cp, net->sw_ln[idx], net->sw_ln[idx] + cp, 1e-5f, s); });
        };
        for (size_t i = 0; i < net->sw_depths.size(); ++i) {
            for (int j = 0; j < net->sw_depths[i]; ++j, ++blk) {
                const f16* x = j == 0 ? r[cur] : t;
                if (int rc = sliced((3 * nh + 1) / 2, x, qkv, 0, nullptr)) return rc;
                if (int rc = plksr_pass(s, "window_attention_cos", 4.0 * 64 * 32 * nh * px, px * nh * 256.0 + nh * 16384.0, 8001, [&] {
                        return win_attn_cos_launch(qkv, G, att, G, net->sw_relb[blk], net->sw_tau[blk], N, Hp, Wp, nh, net->sw_d, (j & 1) ? 4 : 0, s); })) return rc;
                if (int rc = sliced(cp / 64, att, u, 0, nullptr)) return rc;
                if (int rc = norm_add(1 + 2 * blk, u, x, t)) return rc;
                if (int rc = sliced(net->sw_hp / 64, t, hid, 12, nullptr)) return rc;
                if (int rc = sliced(cp / 64, hid, u, 0, nullptr)) return rc;
                if (int rc = norm_add(2 + 2 * blk, u, t, t)) return rc;
            }
            if (int rc = resi(t, r[cur ^ 1], r[cur])) return rc;
            cur ^= 1;
        }
    } else
    for (size_t i = 0; i < net->sw_depths.size(); ++i) {
        for (int j = 0; j < net->sw_depths[i]; ++j, ++blk) {
            const f16* x = j == 0 ? r[cur] : t;
            if (int rc = norm(1 + 2 * blk, x, u)) return rc;
            if (int rc = sliced((3 * nh + 1) / 2, u, qkv, 0, nullptr)) return rc;
            // launch kind 8001: the window attention -- bytes: q, k, v in, o out (32-channel head groups), the bias table
            if (int rc = plksr_pass(s, "window_attention", 4.0 * 64 * 32 * nh * px, px * nh * 256.0 + nh * 16384.0, 8001,
                                    [&] { return win_attn_launch(qkv, G, att, G, net->sw_relb[blk], N, Hp, Wp, nh, net->sw_d, (j & 1) ? 4 : 0, s); })) return rc;
            if (int rc = sliced(cp / 64, att, t, 0, x)) return rc;
            if (int rc = norm(2 + 2 * blk, t, u)) return rc;
            if (int rc = sliced(net->sw_hp / 64, u, hid, 12, nullptr)) return rc;
            if (int rc = sliced(cp / 64, hid, t, 0, t)) return rc;
        }
        if (int rc = resi(t, r[cur ^ 1], r[cur])) return rc;
        cur ^= 1;
    }
    if (int rc = norm((int)net->sw_ln.size() - 1, r[cur], t)) return rc;
    f16* F = r[cur ^ 1];
    if (int rc = resi(t, F, f0)) return rc;

    const int hs = Hp * sc, wsz = Wp * sc;
    void* dst = padded ? (void*)(ws + cv.outp) : d_out;
    if (net->sw_tail == 1) {     // pixelshuffledirect: one conv C -> s^2 out, PixelShuffle(s) as the store (SRVGGNetCompact's tail without a base image)
        const ConvSlot& cl = net->convs[ci++];
        f16* tail = (f16*)(ws + cv.hr);
        ConvLaunch L = mk_launch(cl, F, G, tail, G, N, Hp, Wp, 0, 0);
        L.K = cl.Kp;
        if (int rc = do_conv(L, s)) return rc;
        ShuffleAddLaunch T{};
        T.slab = tail; T.gstride = G; T.base = nullptr;
        T.out = dst; T.out_mode = omode; T.out_denorm = net->u8_normalize;
        T.C = net->out_nc; T.s = sc; T.N = N; T.H = Hp; T.W = Wp;
        const double k = (double)cl.K;
        if (int rc = plksr_pass(s, "shuffle (SwinIR tail)", 0.0, px * (k * 2.0 + k * (omode == 2 ? 1.0 : omode == 1 ? 4.0 : 2.0)), 6000, [&] { return shuffle_add_launch(T, s); })) return rc;
    } else {
        f16* b64 = (f16*)(ws + cv.b64);
        {   // conv_before_upsample + nn.LeakyReLU() (slope 0.01: act 8 with a constant slope vector)
            const ConvSlot& cb = net->convs[ci++];
            ConvLaunch L = mk_launch(cb, F, G, b64, G, N, Hp, Wp, 8, 0);
            L.slope = cb.d_slope;
            if (int rc = do_conv(L, s)) return rc;
        }
        const f16* hr = b64;
        int h = Hp, w = Wp;
        if (net->sw_tail == 0 && sc == 3) {          // conv 64 -> 576, PixelShuffle(3) as a gather pass
            const ConvSlot& cs = net->convs[ci++];
            f16 *Y = (f16*)(ws + cv.up[0]), *D = (f16*)(ws + cv.up[1]);
            if (int rc = do_conv(mk_launch(cs, hr, G, Y, G, N, h, w, 0, 0), s)) return rc;
            // launch kind 8004: the PixelShuffle(3) gather -- bytes: 576 channels in, 64 x 9 pixels out
            if (int rc = plksr_pass(s, "pixel_shuffle3", 0.0, px * 576 * 4.0, 8004, [&] { return launch_pixel_shuffle(Y, G, D, G * 9, 64, N, h, w, 3, s); })) return rc;
            hr = D; h *= 3; w *= 3;
        } else if (net->sw_tail == 0) {              // per factor of 2: conv 64 -> 256 with PixelShuffle(2) as its store
            for (int st = 0; (2 << st) <= sc; ++st) {
                const ConvSlot& cs = net->convs[ci++];
                f16* D = (f16*)(ws + cv.up[st]);
                const long gi = (long)N * h * w * 32;
                ConvLaunch L = mk_launch(cs, hr, gi, D, gi * 4, N, h, w, 0, 0);
                L.out_mode = OUT_SHUFFLE2;
                if (cs.d_ps && (long)N * h * w * 256 < 0x7fffffffL) { L.wpk = (const f16*)cs.d_ps; L.bias = cs.d_bps; L.rowp = 2; }
                if (int rc = do_conv(L, s)) return rc;
                hr = D; h *= 2; w *= 2;
            }
        } else {                                     // nearest+conv: lrelu(conv_up1(nearest2x)), [lrelu(conv_up2(nearest2x)),] lrelu(conv_hr)
            for (int st = 0; (2 << st) <= sc; ++st) {
                const ConvSlot& cs = net->convs[ci++];
                f16* D = (f16*)(ws + cv.up[st]);
                const long gi = (long)N * h * w * 32;
                ConvLaunch L = mk_launch(cs, hr, gi, D, gi * 4, N, 2 * h, 2 * w, 1, 0);
                L.up = 1;
                if (int rc = do_conv(L, s)) return rc;
                hr = D; h *= 2; w *= 2;
            }
            const ConvSlot& ch = net->convs[ci++];
            const long gh = (long)N * h * w * 32;
            f16* D = (f16*)(ws + cv.hr);
            if (int rc = do_conv(mk_launch(ch, hr, gh, D, gh, N, h, w, 1, 0), s)) return rc;
            hr = D;
        }
        const ConvSlot& cl = net->convs[ci++];
        ConvLaunch L = mk_launch(cl, hr, (long)N * h * w * 32, dst, 0, N, h, w, 0, 0);
        L.out_mode = OUT_NCHW; L.out_f32 = out_dtype == INNFER_F32;
        L.out_u8 = out_dtype == INNFER_U8; L.out_denorm = net->u8_normalize; L.out_round16 = 1;
        if (int rc = do_conv(L, s)) return rc;
    }
    if (padded) {
        if (omode == 2) return window("crop", dst, d_out, N, hs, wsz, H * sc, W * sc, net->out_nc, 8003);
        return window("crop", dst, d_out, (long)N * net->out_nc, hs, wsz, H * sc, W * sc, omode == 1 ? 4 : 2, 8003);
    }
    return INNFER_OK;
}

// Launch a dependent chain of same-resolution convs.  band_rows == 0: one launch per
// layer over the whole frame.  band_rows > 0: skewed row bands -- layer l of band b
// covers rows [b*R - l, (b+1)*R - l), so every row a layer reads from its predecessor
// (its own rows +-1) has already been produced, nothing is recomputed, and the ~R-row
// working set of consecutive layers stays resident in the 256 MiB Infinity Cache
// instead of streaming 1664 B/pixel/RDB from HBM.
int run_chain(std::vector<ConvLaunch>& chain, int band_rows, hipStream_t s) {
    if (chain.empty()) return INNFER_OK;
    const int H = chain[0].H, L = (int)chain.size();
    if (band_rows <= 0 || band_rows >= H) {
        for (auto& c : chain) { int rc = do_conv(c, s); if (rc) return rc; }
        return INNFER_OK;
    }
    const int nbands = (H + (L - 1) + band_rows - 1) / band_rows;
    for (int b = 0; b < nbands; ++b)
        for (int l = 0; l < L; ++l) {
            int y0 = b * band_rows - l, y1 = y0 + band_rows;
            if (y0 < 0) y0 = 0;
            if (y1 > H) y1 = H;
            if (b == nbands - 1) y1 = H;
            if (y0 >= y1) continue;
            ConvLaunch c = chain[l];
            c.y0 = y0; c.y1 = y1;
            int rc = do_conv(c, s);
            if (rc) return rc;
        }
    return INNFER_OK;
}

}  // namespace

extern "C" int innfer_net_forward(innfer_net_t net, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                                  int N, int H, int W, void* d_ws, size_t ws_bytes, void* stream) {
    if (!net || !d_in || !d_out || !d_ws) return set_error(INNFER_ERR_INVALID, "forward: null argument");
    if (N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "forward: bad shape %dx%dx%d", N, H, W);
    auto dtype_ok = [](int d) { return d == INNFER_F16 || d == INNFER_F32 || d == INNFER_U8; };
    if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return set_error(INNFER_ERR_INVALID, "forward: bad dtype");
    if (out_dtype == INNFER_U8 && net->out_nc > 4) return set_error(INNFER_ERR_UNSUPPORTED, "forward: a uint8 image has at most 4 channels (out_nc %d)", net->out_nc);
    for (auto& c : net->convs)
        if (!c.loaded) return set_error(INNFER_ERR_INVALID, "forward: weights of '%s' were never set", c.key.c_str());
    const int img_h = H, img_w = W;               // (unshuffle > 1: the image; H x W below is the LR grid every layer runs on)
    H = (H + net->unshuffle - 1) / net->unshuffle; W = (W + net->unshuffle - 1) / net->unshuffle;
    const Carve cv = carve(net, N, H, W);
    if (ws_bytes < cv.total) return set_error(INNFER_ERR_WORKSPACE, "forward: workspace %zu < %zu bytes", ws_bytes, cv.total);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d_ws;
    if (net->kind == 5 || net->kind == 6 || net->kind == 7 || net->kind == 8 || net->kind == 9) return swinir_forward(net, d_in, in_dtype, d_out, out_dtype, N, H, W, ws, s);
    if (net->kind == 2) return compact_forward(net, d_in, in_dtype, d_out, out_dtype, N, H, W, ws, cv, s);
    if (net->kind == 3) return span_forward(net, d_in, in_dtype, d_out, out_dtype, N, H, W, ws, cv, s);
    if (net->kind == 4) return plksr_forward(net, d_in, in_dtype, d_out, out_dtype, N, H, W, ws, cv, s);
    const int nf = net->nf, gc = net->gc;
    const long G = (long)N * H * W * 32;          // group stride of every LR-resolution slab
    const long LO = (long)(cv.lo / 2);            // fp32-accurate mode: elements from a slab to its lo twin (0: fp16 mode)
    if (net->fp32) {
        if (in_dtype == INNFER_F16) return set_error(INNFER_ERR_INVALID, "forward: the fp32-accurate mode takes fp32 or uint8 input (an fp16 tensor is the fp16 mode's)");
        for (auto& c : net->convs)                // built by innfer_net_set_precision(1) (load time); a conv re-set since then rebuilds there too
            if (!c.first && !c.d_w32) return set_error(INNFER_ERR_INVALID, "forward: the fp32-accurate panels of '%s' are missing: call innfer_net_set_precision(net, 1) after the last innfer_net_set_conv", c.key.c_str());
    }
    auto mk = [&](const ConvSlot& cs, const f16* in, long in_g, void* out, long out_g, int N_, int H_, int W_, int act) {
        ConvLaunch L = mk_launch(cs, in, in_g, out, out_g, N_, H_, W_, act, LO);
        L.grid2 = net->kind == 0 ? net->consumer_grid : 0;          // (taken only by the launches that have the form: conv_launch)
        return L;
    };
    f16* fea = (f16*)(ws + cv.fea);
    f16* slab[3] = {(f16*)(ws + cv.slab[0]), (f16*)(ws + cv.slab[1]), (f16*)(ws + cv.slab[2])};
    f16* trunk = (f16*)(ws + cv.trunk);
    int ci = 0;

    if (net->unshuffle > 1) {   // conv_first(pixel_unshuffle(x, r)): the image -> fea + slab[0][0:nf) on the LR grid
        const ConvSlot& c0 = net->convs[ci++];
        FirstUnshuffleLaunch F{};
        F.in = d_in; F.in_f32 = in_dtype == INNFER_F32; F.Cin = net->in_nc; F.r = net->unshuffle; F.wpk = c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = net->u8_round16;
        F.out = fea; F.out_gstride = G; F.out2 = slab[0]; F.out2_gstride = G;
        F.K = nf; F.N = N; F.H = img_h; F.W = img_w; F.act = 0;
        F.out_lo = LO; F.out2_lo = LO;
        int rc = do_first_unshuffle(F, s);
        if (rc) return rc;
    } else {   // conv_first: NCHW input -> fea (+ slab[0][0:nf))
        const ConvSlot& c0 = net->convs[ci++];
        FirstConvLaunch F{};
        F.in = d_in; F.in_f32 = in_dtype == INNFER_F32; F.Cin = c0.C; F.w = (const float*)c0.d_w; F.bias = c0.d_b;
        F.in_u8 = in_dtype == INNFER_U8; F.in_norm = net->u8_normalize; F.in_round16 = net->u8_round16;     // np2tensor as the conv's prologue
        F.out = fea; F.out_gstride = G; F.out2 = slab[0]; F.out2_gstride = G;
        // (SRResNet: the first block reads fea itself -- a second copy in slab[0] only serves the dense blocks' concatenation; one 128 B / pixel store less in a
        //  launch that is bound by its stores)
        if (net->kind == 1 && net->nb > 0) F.out2 = nullptr;
        F.K = nf; F.N = N; F.H = H; F.W = W; F.act = 0;
        F.out_lo = LO; F.out2_lo = LO;
        int rc = do_first(F, s);
        if (rc) return rc;
    }

    std::vector<ConvLaunch> chain;
    int cur = 0;
    if (net->kind == 0) {
        for (int b = 0; b < net->nb; ++b) {
            // three rotating slabs: the RRDB's input stays untouched (its x*0.2 + x residual) while the blocks ping-pong between the other two
            const int in_slab = cur;
            const int f1 = (cur + 1) % 3, f2 = (cur + 2) % 3;
            const int nr = net->nr;
            int last = in_slab;
            for (int r = 0; r < nr; ++r) {
                const int work_r = last, dest_r = (r == 0 || last == f2) ? f1 : f2;
                last = dest_r;
                f16* S = slab[work_r];
                f16* t1x1 = (f16*)(ws + cv.tmp);
                if (net->plus) {                 // t = conv1x1(x): no bias, no activation
                    const ConvSlot& cs = net->convs[ci++];
                    chain.push_back(mk(cs, S, G, t1x1, G, N, H, W, 0));
                }
                for (int i = 0; i < 4; ++i) {
                    const ConvSlot& cs = net->convs[ci++];
                    ConvLaunch L = mk(cs, S, G, S + (long)((nf + i * gc) / 32) * G, G, N, H, W, net->trunk_act);
                    if (net->plus && i == 1) { L.res1 = t1x1; L.res1_gstride = G; L.s1 = 1.f; }          // x2 += conv1x1(x)
                    if (net->plus && i == 3) {                                                             // x4 += x2
                        L.res1 = S + (long)((nf + gc) / 32) * G; L.res1_gstride = G; L.s1 = 1.f;
                    }
                    chain.push_back(L);
                }
                const ConvSlot& cs = net->convs[ci++];
                ConvLaunch L = mk(cs, S, G, slab[dest_r], G, N, H, W, 0);
                L.res1 = S; L.res1_gstride = G; L.s1 = 0.2f;                      // x5*0.2 + x
                L.res1_lds = net->res_lds;                                        // ... with x from the conv's own LDS stages where the kernel has that form (fp16 engine, nf 64)
                if (r == nr - 1) { L.res2 = slab[in_slab]; L.res2_gstride = G; L.s2 = 0.2f; }   // RRDB: out*0.2 + x
                chain.push_back(L);
            }
            cur = last;
        }
    } else {
        // SRGAN residual blocks: t = t + conv(relu(conv(t))) on nf-wide slabs
        for (int b = 0; b < net->nb; ++b) {
            const int a = cur, m = (cur + 1) % 3, o = (cur + 2) % 3;
            const ConvSlot& c0 = net->convs[ci++];
            const f16* xa = b == 0 ? fea : slab[a];                  // the block's input (block 0: conv_first's output, never rewritten: the last shortcut reads it too)
            const f16* in0 = xa;
            if (c0.d_map) {          // mode 'NAC': norm -> act in front of the conv, into the (still unused) trunk slab; launches in order, whole frame
                int rc = run_chain(chain, 0, s);
                if (rc) return rc;
                chain.clear();
                rc = do_input_map(c0, xa, trunk, G, s, LO);
                if (rc) return rc;
                in0 = trunk;
            }
            chain.push_back(mk(c0, in0, G, slab[m], G, N, H, W, net->trunk_act));
            const ConvSlot& c1 = net->convs[ci++];
            ConvLaunch L = mk(c1, slab[m], G, slab[o], G, N, H, W, 0);
            L.res1 = xa; L.res1_gstride = G; L.s1 = net->res_scale;               // x + res * res_scale
            chain.push_back(L);
            cur = o;
        }
    }
    {   // trunk conv + ShortcutBlock: fea + conv(t)
        const ConvSlot& cs = net->convs[ci++];
        const f16* in = slab[cur];
        if (cs.d_map) {
            int rc = run_chain(chain, 0, s);
            if (rc) return rc;
            chain.clear();
            rc = do_input_map(cs, slab[cur], slab[(cur + 1) % 3], G, s, LO);
            if (rc) return rc;
            in = slab[(cur + 1) % 3];
        }
        ConvLaunch L = mk(cs, in, G, trunk, G, N, H, W, 0);
        L.res1 = fea; L.res1_gstride = G; L.s1 = 1.f;
        chain.push_back(L);
    }
    bool any_map = false;
    for (auto& c : net->convs) any_map |= c.d_map != nullptr;
    int rc = run_chain(chain, (any_map || net->fp32) ? 0 : net->band_rows, s);
    if (rc) return rc;

    const f16* t = trunk;
    int h = H, w = W;
    for (int u = 0; u < net->n_up; ++u) {
        const ConvSlot& cs = net->convs[ci++];
        f16* dst = (f16*)(ws + cv.up[u]);
        const long gi = (long)N * h * w * 32, go = gi * 4;
        if (net->ps_up && (net->scale == 3 || net->nf != 64 || net->fp32)) {
            // PixelShuffle(3), or factor 2 on 32 features: the conv (nf -> r^2 nf, act in its epilogue -- it commutes with the permutation) writes a
            // slab in the (still unused) HR region, one gather pass rearranges it (block.py:333-346).  The 64-feature factor-2 stages shuffle in the
            // conv's own store (OUT_SHUFFLE2) below.
            const int r = net->scale == 3 ? 3 : 2;
            f16* Y = (f16*)(ws + cv.hr);
            rc = do_conv(mk(cs, t, gi, Y, gi, N, h, w, net->trunk_act), s);
            if (rc) return rc;
            rc = launch_pixel_shuffle(Y, gi, dst, gi * r * r, net->nf, N, h, w, r, s, LO);
            if (rc) return rc;
            t = dst; h *= r; w *= r;
            continue;
        }
        if (net->scale == 3) {      // Upsample(nearest 3x), materialised in the (still unused) HR slab -> conv -> LeakyReLU
            f16* U = (f16*)(ws + cv.hr);
            const long g3 = gi * 9;
            rc = launch_upsample_nearest(t, gi, U, g3, net->nf / 32, N, h, w, 3, s, LO);
            if (rc) return rc;
            rc = do_conv(mk(cs, U, g3, dst, g3, N, 3 * h, 3 * w, net->trunk_act), s);
            if (rc) return rc;
            t = dst; h *= 3; w *= 3;
            continue;
        }
        if (u == net->n_up - 1 && !net->ps_up && net->up_phases == 1 && net->hr_chain && !net->fp32 && cs.d_up4p && !cs.d_map && (net->trunk_act == 1 || net->trunk_act == 2) && w > 16 &&
            net->fused_tail && !any_map && net->band_rows == 0 && net->final_act == 0 && net->outm == 0) {
            // The last upconv_block -> HR_conv0 -> conv_last as ONE kernel (hr_chain.hip): the [64 ch, 2h x 2w] tensor between them (4.25 GB of a 1080p -> 4K frame, written
            // by a store-bound launch and read back by the next) stays in LDS tile by tile.  Same operands in the same order per value as the two launches below: same bits.
            const ConvSlot& ch = net->convs[ci];           // HR_conv0
            const ConvSlot& cl = net->convs[ci + 1];       // conv_last
            const int hh = 2 * h, wh = 2 * w;
            const long gh = (long)N * hh * wh * 32;
            if (ch.K == 64 && ch.C == 64 && ch.rowp && cl.d_fuse && cl.loaded && conv_fuse_side_bytes(N, hh, wh) <= (size_t)gh * 2 * (net->nf / 32)) {
                ConvLaunch L = mk(ch, nullptr, gh, ws + cv.hr, gh, N, hh, wh, net->trunk_act);
                L.fuse_w = (const f16*)cl.d_fuse; L.fuse_bias = cl.d_b; L.fuse_side = (float*)(ws + cv.hr); L.fuse_out = d_out; L.fuse_oc = cl.K;
                L.fuse_out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0;
                L.out_denorm = net->u8_normalize; L.out_round16 = net->u8_round16;
                if (hr_chain_ok(L)) {
                    rc = timed_begin(s);
                    if (rc) return rc;
                    {
                        thread_local unsigned parity = 0;
                        L.rev = INNFER_KNOB("INNFER_TILE_REV", 1) ? (int)(parity++ & 1) : 0;
                    }
                    rc = hr_chain_launch(L, t, gi, (const f16*)cs.d_up4p, cs.d_b4, net->trunk_act, s);
                    if (rc) return rc;
                    rc = debug_after("hr_chain", s);
                    if (rc) return rc;
                    // the three layers' ALGORITHMIC FLOPs (nine taps each on the HR grid); bytes: the LR tensor in, the planar result out, the weights
                    const double pxh = (double)N * hh * wh;
                    const double ob = L.fuse_out_mode == 2 ? 1.0 : L.fuse_out_mode == 1 ? 4.0 : 2.0;
                    return timed_end(s, 2.0 * 9.0 * (64.0 * 64 + 64.0 * 64 + 64.0 * cl.K) * pxh, pxh / 4 * 128.0 + pxh * cl.K * ob + 9.0 * (2 * 64.0 * 64 + 64.0 * cl.K) * 2.0, 5000 + 16 * 4);
                }
            }
        }
        if (!net->ps_up && net->up_phases && !net->fp32 && cs.d_up4 && !cs.d_map && net->trunk_act <= 2) {
            // Upsample(nearest 2x) -> conv -> act as the four output phases of the equivalent transposed conv: 2x2 taps on the LR grid instead of 3x3 on the
            // HR grid (2.25 x fewer MACs), on the phase-lattice instantiation (conv3x3_pc<.., TM = TAPS_PHASE>)
            ConvLaunch L = mk(cs, t, gi, dst, go, N, h, w, net->trunk_act);
            const bool one_visit = net->up_phases == 1 && cs.d_up4p && w > 16;       // all four phases in one visit of a tile (C = 64, plane-order panels); else one phase per visit
            L.wpk = (const f16*)(one_visit ? cs.d_up4p : cs.d_up4); L.bias = cs.d_b4;
            L.K = 4 * cs.K; L.phase_c = cs.K; L.deconv_phases = one_visit ? 1 : 2; L.rowp = one_visit ? 1 : 0;
            rc = do_conv(L, s);
        } else if (!net->ps_up) {    // Upsample(nearest 2x) -> conv -> act
            ConvLaunch L = mk(cs, t, gi, dst, go, N, 2 * h, 2 * w, net->trunk_act);
            L.up = 1;
            rc = do_conv(L, s);
        } else {                     // conv nf->4nf -> PixelShuffle(2) -> act (SRGAN: ReLU; RRDBNet(upsample_mode='pixelshuffle'): its act_type)
            ConvLaunch L = mk(cs, t, gi, dst, go, N, h, w, net->trunk_act);
            L.out_mode = OUT_SHUFFLE2;
            // the store of the producer / consumer kernel (conv3x3_pc PSH) while an output group stays below 2 GiB (conv_launch's bound for that form: chop batches of
            // more than 209 tiles of 200 x 200 at the first stage and 4x frames beyond 8.39 M LR pixels at the second take the two-workgroup kernel, whose indices are 64-bit)
            if (cs.d_ps && !cs.d_map && (long)N * h * w * 256 < 0x7fffffffL) { L.wpk = (const f16*)cs.d_ps; L.bias = cs.d_bps; L.rowp = 2; }
            rc = do_conv(L, s);
        }
        if (rc) return rc;
        t = dst; h *= 2; w *= 2;
    }
    {
        const ConvSlot& cs = net->convs[ci++];
        const long gh = (long)N * h * w * 32;
        ConvLaunch L = mk(cs, t, gh, ws + cv.hr, gh, N, h, w, net->trunk_act);
        // HR_conv0 -> conv_last in one kernel (conv3x3.hip, FUSE) where the shapes allow it: fp16 engine, 64 features, <= 3 planar float outputs without final
        // activation / outm, whole 16 x 32 tiles.  The rim buffer lives where the HR slab would have been.
        const ConvSlot& cl = net->convs[ci];
        if (net->fused_tail && !net->fp32 && !any_map && net->band_rows == 0 && cl.d_fuse && cl.loaded && net->final_act == 0 && net->outm == 0 &&
            (out_dtype == INNFER_F16 || out_dtype == INNFER_F32 || out_dtype == INNFER_U8) && conv_fuse_side_bytes(N, h, w) <= (size_t)gh * 2 * (net->nf / 32)) {
            L.fuse_w = (const f16*)cl.d_fuse; L.fuse_bias = cl.d_b; L.fuse_side = (float*)(ws + cv.hr); L.fuse_out = d_out; L.fuse_oc = cl.K;
            L.fuse_out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0;
            L.out_denorm = net->u8_normalize; L.out_round16 = net->u8_round16;     // (uint8: tensor2np as the store, as in the two-launch form)
            if (conv_fuse_last_ok(L)) {
                rc = do_conv(L, s);
                if (rc) return rc;
                return INNFER_OK;
            }
            L.fuse_w = nullptr;
        }
        rc = do_conv(L, s);
        if (rc) return rc;
    }
    {
        const ConvSlot& cs = net->convs[ci++];
        ConvLaunch L = mk(cs, (const f16*)(ws + cv.hr), (long)N * h * w * 32, d_out, 0, N, h, w, net->final_act);
        L.out_mode = OUT_NCHW; L.out_f32 = out_dtype == INNFER_F32;
        L.outm = net->outm;
        L.out_u8 = out_dtype == INNFER_U8; L.out_denorm = net->u8_normalize; L.out_round16 = net->u8_round16;     // tensor2np as the conv's epilogue
        rc = do_conv(L, s);
        if (rc) return rc;
    }
    return INNFER_OK;
}

extern "C" int innfer_net_forward_timed(innfer_net_t net, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                                        int N, int H, int W, void* d_ws, size_t ws_bytes, void* stream,
                                        int cap, float* h_ms, double* h_flops, double* h_bytes, int* h_kind, int* n_launches) {
    LaunchTimer t;
    g_timer = &t;
    int rc = innfer_net_forward(net, d_in, in_dtype, d_out, out_dtype, N, H, W, d_ws, ws_bytes, stream);
    g_timer = nullptr;
    if (rc == INNFER_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        rc = set_error(INNFER_ERR_HIP, "forward_timed: stream synchronize failed");
    const int n = (int)t.flops.size();
    if (rc == INNFER_OK) {
        if (n_launches) *n_launches = n;
        for (int i = 0; i < n && i < cap; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]);
            if (h_ms) h_ms[i] = ms;
            if (h_flops) h_flops[i] = t.flops[i];
            if (h_bytes) h_bytes[i] = t.bytes[i];
            if (h_kind) h_kind[i] = t.kind[i];
        }
    }
    for (auto e : t.ev) (void)hipEventDestroy(e);
    return rc;
}

// ---------------------------------------------------------------- single conv
extern "C" size_t innfer_conv3x3_packed_bytes(int K, int C) {
    if (K <= 0 || C <= 0 || C % 32) return 0;
    return conv_packed_bytes(K, C);
}

extern "C" int innfer_pack_conv3x3(const float* w, int K, int C, void* h_packed) {
    if (!w || !h_packed || K <= 0 || C <= 0 || C % 32)
        return set_error(INNFER_ERR_INVALID, "pack_conv3x3: K=%d C=%d (C must be a multiple of 32)", K, C);
    conv_pack(w, K, C, h_packed);
    return INNFER_OK;
}

extern "C" int innfer_pack_conv3x3_rows(const float* w, int K, int C, int plane_rows, void* h_packed) {
    if (!w || !h_packed || K <= 0 || C <= 0 || C % 32 || (plane_rows && K % 64))
        return set_error(INNFER_ERR_INVALID, "pack_conv3x3_rows: K=%d C=%d (C must be a multiple of 32; the plane row order needs K %% 64 == 0)", K, C);
    conv_pack(w, K, C, h_packed, plane_rows ? 1 : 0);
    return INNFER_OK;
}

extern "C" int innfer_pack_conv3x3_shuffle2(const float* w, const float* bias, int K, int C, void* h_packed, float* h_bias_out) {
    if (!w || !h_packed || !h_bias_out || K <= 0 || K % 256 || C <= 0 || C % 32)
        return set_error(INNFER_ERR_INVALID, "pack_conv3x3_shuffle2: K=%d C=%d (K must be a multiple of 256: four phases of 64-channel groups; C of 32)", K, C);
    conv_pack_shuffle2(w, bias, K, C, h_packed, h_bias_out);
    return INNFER_OK;
}

extern "C" int innfer_pack_convt2x_rows(const float* w, int K, int C, int k, int plane_rows, void* packed) {
    if (!w || !packed || K <= 0 || K % 64 || C <= 0 || C % 32 || (k != 3 && k != 4)) return set_error(INNFER_ERR_INVALID, "pack_convT2x_rows: K=%d (%% 64) C=%d (%% 32) k=%d (3 | 4)", K, C, k);
    conv_pack_deconv2x(w, K, C, k, packed, plane_rows ? 1 : 0);
    return INNFER_OK;
}

extern "C" int innfer_pack_conv3x3_split(const float* w, int K, int C, void* h_packed) {
    if (!w || !h_packed || K <= 0 || C <= 0 || C % 32)
        return set_error(INNFER_ERR_INVALID, "pack_conv3x3_split: K=%d C=%d (C must be a multiple of 32)", K, C);
    conv_pack_split(w, K, C, h_packed);
    return INNFER_OK;
}

extern "C" size_t innfer_conv7x1_packed_bytes(int K, int C) { return (K > 0 && C > 0 && C % 32 == 0) ? conv_packed_bytes7v(K, C) : 0; }
extern "C" int innfer_pack_conv7x1(const float* w, int K, int C, void* packed) {
    if (!w || !packed || K <= 0 || K % 32 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_conv7x1: K=%d (%% 32) C=%d (%% 32)", K, C);
    conv_pack7v(w, K, C, packed);
    return INNFER_OK;
}
extern "C" size_t innfer_conv4x4s2_packed_bytes(int K, int C) { return (K > 0 && C > 0 && C % 32 == 0) ? conv_packed_bytes_s2k4(K, C) : 0; }
extern "C" int innfer_pack_conv4x4s2(const float* w, int K, int C, void* packed) {
    if (!w || !packed || K <= 0 || K % 64 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_conv4x4s2: K=%d (%% 64) C=%d (%% 32)", K, C);
    conv_pack_s2k4(w, K, C, packed);
    return INNFER_OK;
}
extern "C" size_t innfer_convt2x_packed_bytes(int K, int C) { return (K > 0 && C > 0 && C % 32 == 0) ? conv_packed_bytes_deconv2x(K, C) : 0; }
extern "C" int innfer_pack_convt2x(const float* w, int K, int C, int k, void* packed) {
    if (!w || !packed || K <= 0 || K % 64 || C <= 0 || C % 32 || (k != 3 && k != 4)) return set_error(INNFER_ERR_INVALID, "pack_convT2x: K=%d (%% 64) C=%d (%% 32) k=%d (3 | 4)", K, C, k);
    conv_pack_deconv2x(w, K, C, k, packed);
    return INNFER_OK;
}

// (121) the panels of the forms innfer_conv_args reaches since then
extern "C" size_t innfer_conv1x1_packed_bytes(int K, int C) { return (K > 0 && C > 0 && C % 32 == 0) ? conv_packed_bytes_taps(K, C, TAPS_1X1) : 0; }
extern "C" int innfer_pack_conv1x1(const float* w, int K, int C, void* packed) {
    if (!w || !packed || K <= 0 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_conv1x1: K=%d C=%d (%% 32)", K, C);
    conv_pack_1x1(w, K, C, packed);
    return INNFER_OK;
}
extern "C" int innfer_pack_conv1x1_split(const float* w, int K, int C, void* packed) {
    if (!w || !packed || K <= 0 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_conv1x1_split: K=%d C=%d (%% 32)", K, C);
    conv_pack_1x1_split(w, K, C, packed);
    return INNFER_OK;
}
extern "C" int innfer_pack_selfgate(const float* w32x32, void* packed_2k) {
    if (!w32x32 || !packed_2k) return set_error(INNFER_ERR_INVALID, "pack_selfgate: null argument");
    conv_pack_selfgate(w32x32, packed_2k);
    return INNFER_OK;
}
extern "C" size_t innfer_conv7x7_packed_bytes(int K, int C) { return (K > 0 && C > 0 && C % 32 == 0) ? conv_packed_bytes7x7(K, C) : 0; }
extern "C" int innfer_pack_conv7x7(const float* w, int K, int C, void* packed) {
    if (!w || !packed || K <= 0 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_conv7x7: K=%d C=%d (%% 32)", K, C);
    conv_pack7x7(w, K, C, packed);
    return INNFER_OK;
}
extern "C" int innfer_pack_up2x_phases(const float* w, int K, int C, int plane_rows, void* packed) {
    if (!w || !packed || K <= 0 || K % 64 || C <= 0 || C % 32) return set_error(INNFER_ERR_INVALID, "pack_up2x_phases: K=%d (%% 64) C=%d (%% 32)", K, C);
    conv_pack_up2x_phases(w, K, C, packed, plane_rows ? 1 : 0);
    return INNFER_OK;
}

// innfer_conv_args.d_stats_part -> ConvLaunch.stats_part, behind the size check (conv_launch decides which forms take statistics)
static int conv_args_stats(const innfer_conv_args* a, int phases, ConvLaunch& L) {
    if (!a->d_stats_part) return INNFER_OK;
    if (a->N <= 0 || a->H <= 0 || a->W <= 0 || a->K <= 0) return set_error(INNFER_ERR_INVALID, "conv3x3: statistics of an empty launch (N=%d H=%d W=%d K=%d)", a->N, a->H, a->W, a->K);
    const long long need = (long long)a->N * conv_stats_nper(a->H, a->W, phases) * a->K * 3;
    if ((long long)a->stats_part_floats < need)
        return set_error(INNFER_ERR_WORKSPACE, "conv3x3: stats_part_floats %lld < %lld (N * records * channels * 3)", (long long)a->stats_part_floats, need);
    L.stats_part = a->d_stats_part;
    return INNFER_OK;
}

extern "C" int innfer_conv_stats_records(int H, int W, int phases) {
    if (H <= 0 || W <= 0 || (phases != 1 && phases != 4)) return set_error(INNFER_ERR_INVALID, "conv_stats_records: H=%d W=%d phases=%d (1 | 4)", H, W, phases);
    return conv_stats_nper(H, W, phases);
}

extern "C" int innfer_norm_combine_parts(const float* d_part, int nper, int64_t HW, float eps, const float* d_gamma, const float* d_beta, float* d_alpha, float* d_shift,
                                         int C, int N, void* stream) {
    if (!d_part || !d_alpha || !d_shift || nper <= 0 || HW <= 0 || C <= 0 || N <= 0 || N > 65535)
        return set_error(INNFER_ERR_INVALID, "norm_combine_parts: null argument or nper=%d HW=%lld C=%d N=%d", nper, (long long)HW, C, N);
    return norm::launch_combine_parts(d_part, nper, (long)HW, eps, d_gamma, d_beta, d_alpha, d_shift, C, N, (hipStream_t)stream);
}

extern "C" int innfer_norm_stats(const void* d_src, int slab, int64_t gs, int cpad, int64_t HW, float eps, const float* d_gamma, const float* d_beta, float* d_alpha,
                                 float* d_shift, int C, int N, float* d_part, int64_t part_floats, void* stream) {
    if (!d_src || !d_alpha || !d_shift || HW <= 0 || C <= 0 || N <= 0 || N > 65535 || (HW + norm::SEG - 1) / norm::SEG > 65535)
        return set_error(INNFER_ERR_INVALID, "norm_stats: null argument or HW=%lld C=%d N=%d", (long long)HW, C, N);
    if (slab ? gs < (int64_t)N * HW * 32 : (cpad < C || cpad % 32))
        return set_error(INNFER_ERR_INVALID, "norm_stats: group stride %lld < N * HW * 32 (slab), or cpad=%d below C=%d / not a multiple of 32 (fp32)", (long long)gs, cpad, C);
    if (HW > norm::SEG && (!d_part || part_floats < 0 || (unsigned long long)part_floats < (unsigned long long)N * norm::part_floats(C, (long)HW)))
        return set_error(INNFER_ERR_WORKSPACE, "norm_stats: part_floats %lld < %llu", (long long)part_floats, (unsigned long long)N * norm::part_floats(C, (long)HW));
    return slab ? norm::launch_stats_slab((const f16*)d_src, (long)gs, (long)HW, eps, d_gamma, d_beta, d_alpha, d_shift, C, N, d_part, (hipStream_t)stream)
                : norm::launch_stats((const float*)d_src, cpad, (long)HW, eps, d_gamma, d_beta, d_alpha, d_shift, C, N, d_part, (hipStream_t)stream);
}

static int conv3x3_f16_impl(const innfer_conv_args* a, const float* d_slope, void* stream, int consumer_grid = 1);
extern "C" int innfer_conv3x3_f16(const innfer_conv_args* a, void* stream) { return conv3x3_f16_impl(a, nullptr, stream); }
extern "C" int innfer_conv3x3_f16_grid(const innfer_conv_args* a, int consumer_grid, void* stream) {
    if (consumer_grid < 0 || consumer_grid > 1) return set_error(INNFER_ERR_INVALID, "conv3x3: consumer_grid is 1 (the 2 x 4 consumer grid where the launch has that form) or 0 (the 8 x 1 form)");
    return conv3x3_f16_impl(a, nullptr, stream, consumer_grid);
}
// The same launch with act = 8: f >= 0 ? f : d_slope[c] * f, d_slope padded like d_bias (for tests; the SRVGGNetCompact engine's layers)
extern "C" int innfer_conv3x3_f16_slope(const innfer_conv_args* a, const float* d_slope, void* stream) { return conv3x3_f16_impl(a, d_slope, stream); }

// SwinIR's window attention alone, for tests: win_attn_launch, the code the network runs.  Uploads the bias table, launches, waits.
extern "C" int innfer_window_attention(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads, int head_dim,
                                       int shift, void* stream) {
    if (!d_qkv || !d_out || !h_bias) return set_error(INNFER_ERR_INVALID, "window_attention: null argument");
    if (num_heads < 1 || num_heads > 8) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention: %d heads (built: 1 .. 8)", num_heads);
    Upload b("window_attention", {{h_bias, (size_t)num_heads * 4096}}, "bias table");
    int rc = b.rc;
    if (rc == INNFER_OK) rc = win_attn_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, b.d, N, Hp, Wp, num_heads, head_dim, shift, (hipStream_t)stream);
    return finish("window_attention", rc, stream);
}

// HAT's 16 x 16 window attention alone (key window 16: self, shift 0 | 8; 24: overlapping), for tests: win_attn16_launch, the code the network runs.  Uploads, launches, waits.
extern "C" int innfer_window_attention16(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads, int head_dim,
                                         int shift, int key_window, void* stream) {
    if (!d_qkv || !d_out || !h_bias) return set_error(INNFER_ERR_INVALID, "window_attention16: null argument");
    if (num_heads < 1 || num_heads > 8) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16: %d heads (built: 1 .. 8)", num_heads);
    if (key_window != 16 && key_window != 24) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16: a key window of %d (built: 16, 24)", key_window);
    Upload b("window_attention16", {{h_bias, (size_t)num_heads * 256 * key_window * key_window}}, "bias table");
    int rc = b.rc;
    if (rc == INNFER_OK) rc = win_attn16_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, b.d, N, Hp, Wp, num_heads, head_dim, shift, key_window, (hipStream_t)stream);
    return finish("window_attention16", rc, stream);
}

// DRCT's 16 x 16 window attention for heads of 33 .. 128 channels alone, for tests: win_attn16_wide_launch, the code the network runs.  Every refusal comes before the upload:
// a refused call touches no device memory.  Uploads, launches, waits.
extern "C" int innfer_window_attention16_wide(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads,
                                              int head_dim, int shift, void* stream) {
    if (!d_qkv || !d_out || !h_bias) return set_error(INNFER_ERR_INVALID, "window_attention16_wide: null argument");
    if (num_heads < 1 || num_heads > 8) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16_wide: %d heads (built: 1 .. 8)", num_heads);
    if (head_dim <= 32) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16_wide: heads of %d channels (built: 33 .. 128; innfer_window_attention16 takes <= 32)", head_dim);
    if (head_dim > 128) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16_wide: heads of %d channels (built: 33 .. 128)", head_dim);
    if (N <= 0 || Hp <= 0 || Wp <= 0 || (Hp & 15) || (Wp & 15)) return set_error(INNFER_ERR_INVALID, "window_attention16_wide: %d images of %d x %d (whole 16 x 16 windows)", N, Hp, Wp);
    if (shift != 0 && shift != 8) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention16_wide: shift %d (built: 0, 8)", shift);
    Upload b("window_attention16_wide", {{h_bias, (size_t)num_heads * 65536}}, "bias table");
    int rc = b.rc;
    if (rc == INNFER_OK) rc = win_attn16_wide_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, b.d, N, Hp, Wp, num_heads, head_dim, shift, (hipStream_t)stream);
    return finish("window_attention16_wide", rc, stream);
}

// The holed LayerNorm of DRCT's dense slab alone, for tests: layer_norm_holed_launch, the code the network runs.  h_gamma / h_beta: c_pad host floats in slab order.
extern "C" int innfer_layer_norm_holed(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_end, int c_pad, const float* h_gamma,
                                       const float* h_beta, float eps, void* stream) {
    if (!d_in || !d_out || !h_gamma || !h_beta) return set_error(INNFER_ERR_INVALID, "layer_norm_holed: null argument");
    if (c_pad < 64 || c_pad > 512) return set_error(INNFER_ERR_UNSUPPORTED, "layer_norm_holed: a slab of %d channels (built: 64 .. 512)", c_pad);
    Upload p("layer_norm_holed", {{h_gamma, (size_t)c_pad}, {h_beta, (size_t)c_pad}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = layer_norm_holed_launch((const f16*)d_in, (long)in_gs, (f16*)d_out, (long)out_gs, (long)npix, C, c_end, c_pad, p.d, p.d + c_pad, eps, (hipStream_t)stream);
    return finish("layer_norm_holed", rc, stream);
}

// HAT's channel attention alone, for tests (chan_attn.hip, the code the network runs): the channel sums + the squeeze / excite vector, and the scale-add pass.
extern "C" size_t innfer_chan_attn_work_bytes(int N, int64_t HW, int c_pad) { return (N > 0 && HW > 0 && c_pad > 0) ? ca_work_floats(N, (long)HW, c_pad) * sizeof(float) : 0; }
extern "C" int innfer_chan_attn_excite(const void* d_z, int64_t z_gs, int N, int64_t HW, int C, int c_pad, int hidden, const float* h_w1, const float* h_b1, const float* h_w2,
                                       const float* h_b2, void* d_y, void* d_sums, void* d_work, size_t work_bytes, void* stream) {
    if (!d_z || !h_w1 || !h_b1 || !h_w2 || !h_b2 || !d_y || !d_work) return set_error(INNFER_ERR_INVALID, "chan_attn_excite: null argument");
    if (N <= 0 || HW <= 0 || C < 1 || C > 256 || c_pad < C || c_pad > 256 || c_pad % 64 || hidden < 1 || hidden > 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "chan_attn_excite: N=%d HW=%ld C=%d c_pad=%d hidden=%d (built: C <= c_pad in 64, 128, 192, 256; hidden <= 64)", N, (long)HW, C, c_pad, hidden);
    if (work_bytes < innfer_chan_attn_work_bytes(N, HW, c_pad)) return set_error(INNFER_ERR_WORKSPACE, "chan_attn_excite: work buffer %zu < %zu bytes", work_bytes, innfer_chan_attn_work_bytes(N, HW, c_pad));
    Upload p("chan_attn_excite", {{h_w1, (size_t)hidden * C}, {h_b1, (size_t)hidden}, {h_w2, (size_t)C * hidden}, {h_b2, (size_t)C}}, "weights");
    int rc = p.rc;
    hipStream_t s = (hipStream_t)stream;
    if (rc == INNFER_OK) rc = ca_pool_launch((const f16*)d_z, (long)z_gs, N, (long)HW, c_pad, (float*)d_work, s);
    if (rc == INNFER_OK) rc = ca_excite_launch((const float*)d_work, N, (long)HW, C, c_pad, hidden, p.d, p.d + (size_t)hidden * C, p.d + (size_t)hidden * C + hidden,
                                               p.d + 2 * (size_t)hidden * C + hidden, (float*)d_y, (float*)d_sums, s);
    return finish("chan_attn_excite", rc, stream);
}
extern "C" int innfer_chan_attn_scale_add(void* d_t, int64_t t_gs, const void* d_z, int64_t z_gs, const void* d_y, float conv_scale, int N, int64_t HW, int c_pad, void* stream) {
    if (!d_t || !d_z || !d_y) return set_error(INNFER_ERR_INVALID, "chan_attn_scale_add: null argument");
    int rc = ca_scale_add_launch((f16*)d_t, (long)t_gs, (const f16*)d_z, (long)z_gs, (const float*)d_y, conv_scale, N, (long)HW, c_pad, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "chan_attn_scale_add: the launch failed");
    return rc;
}

// SwinIR's per-pixel LayerNorm alone, for tests: layer_norm_launch, the code the network runs.  Uploads gamma / beta, launches, waits.
extern "C" int innfer_layer_norm(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad, const float* h_gamma, const float* h_beta,
                                 float eps, void* stream) {
    if (!d_in || !d_out || !h_gamma || !h_beta) return set_error(INNFER_ERR_INVALID, "layer_norm: null argument");
    if (C < 1 || C > 256) return set_error(INNFER_ERR_UNSUPPORTED, "layer_norm: C=%d (built: 1 .. 256)", C);
    Upload p("layer_norm", {{h_gamma, (size_t)C}, {h_beta, (size_t)C}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = layer_norm_launch((const f16*)d_in, (long)in_gs, (f16*)d_out, (long)out_gs, (long)npix, C, c_pad, p.d, p.d + C, eps, (hipStream_t)stream);
    return finish("layer_norm", rc, stream);
}

// Swin2SR's cosine window attention alone, for tests: win_attn_cos_launch, the code the network runs.  Uploads the bias table and the per-head scales, launches, waits.
extern "C" int innfer_window_attention_cos(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, const float* h_tau, int N, int Hp, int Wp,
                                           int num_heads, int head_dim, int shift, void* stream) {
    if (!d_qkv || !d_out || !h_bias || !h_tau) return set_error(INNFER_ERR_INVALID, "window_attention_cos: null argument");
    if (num_heads < 1 || num_heads > 8) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention_cos: %d heads (built: 1 .. 8)", num_heads);
    Upload b("window_attention_cos", {{h_bias, (size_t)num_heads * 4096}, {h_tau, (size_t)num_heads}}, "bias table and the scales");
    int rc = b.rc;
    if (rc == INNFER_OK) rc = win_attn_cos_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, b.d, b.d + (size_t)num_heads * 4096, N, Hp, Wp, num_heads, head_dim, shift,
                                                  (hipStream_t)stream);
    return finish("window_attention_cos", rc, stream);
}

// Swin2SR's LayerNorm + residual alone, for tests: layer_norm_add_launch, the code the network runs.  Uploads gamma / beta, launches, waits.
extern "C" int innfer_layer_norm_add(const void* d_in, int64_t in_gs, const void* d_res, int64_t res_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad,
                                     const float* h_gamma, const float* h_beta, float eps, void* stream) {
    if (!d_in || !d_res || !d_out || !h_gamma || !h_beta) return set_error(INNFER_ERR_INVALID, "layer_norm_add: null argument");
    if (C < 1 || C > 256) return set_error(INNFER_ERR_UNSUPPORTED, "layer_norm_add: C=%d (built: 1 .. 256)", C);
    Upload p("layer_norm_add", {{h_gamma, (size_t)C}, {h_beta, (size_t)C}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = layer_norm_add_launch((const f16*)d_in, (long)in_gs, (const f16*)d_res, (long)res_gs, (f16*)d_out, (long)out_gs, (long)npix, C, c_pad, p.d, p.d + C, eps,
                                                    (hipStream_t)stream);
    return finish("layer_norm_add", rc, stream);
}

// RealPLKSR's partial large-kernel conv alone, for tests: plk_pack + plk_conv_launch, the code the network runs.  Uploads, launches, waits.
extern "C" int innfer_plk_conv(const void* d_in, void* d_out, int N, int H, int W, int k, const float* h_weight_oihw, const float* h_bias, void* stream) {
    if (!d_in || !d_out || !h_weight_oihw) return set_error(INNFER_ERR_INVALID, "plk_conv: null argument");
    if (k < 3 || k > 17 || !(k & 1)) return set_error(INNFER_ERR_UNSUPPORTED, "plk_conv: kernel size %d (built: odd, 3 .. 17)", k);
    if (N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "plk_conv: bad shape %dx%dx%d", N, H, W);
    {
        const long G = (long)N * H * W * 32;
        const f16 *a = (const f16*)d_in, *b = (const f16*)d_out;
        if (a < b + G && b < a + G) return set_error(INNFER_ERR_INVALID, "plk_conv: the output group overlaps the input group");
    }
    std::vector<char> host(plk_packed_bytes(k));
    plk_pack(h_weight_oihw, k, host.data());
    float bias[16];
    for (int i = 0; i < 16; ++i) bias[i] = h_bias ? h_bias[i] : 0.f;
    void* d_w = nullptr; float* d_b = nullptr;
    int rc = INNFER_OK;
    if (hipMalloc(&d_w, host.size()) != hipSuccess || hipMalloc((void**)&d_b, sizeof bias) != hipSuccess) rc = set_error(INNFER_ERR_NOMEM, "plk_conv: out of device memory");
    if (rc == INNFER_OK && (hipMemcpy(d_w, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_b, bias, sizeof bias, hipMemcpyHostToDevice) != hipSuccess))
        rc = set_error(INNFER_ERR_HIP, "plk_conv: copying the weights failed");
    if (rc == INNFER_OK) {
        const PlkLaunch P{(const f16*)d_in, (f16*)d_out, (const f16*)d_w, d_b, k, N, H, W};
        rc = plk_conv_launch(P, (hipStream_t)stream);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "plk_conv: the launch failed");
    }
    (void)hipFree(d_w); (void)hipFree(d_b);
    return rc;
}

// GroupNorm(groups, 64) per sample + skip alone, for tests: the three launches of group_norm.hip in the network's order.  Uploads gamma / beta, launches, waits.
extern "C" size_t innfer_group_norm_skip_work_bytes(int N, int64_t HW) { return (N > 0 && HW > 0) ? gn_work_floats(N, (long)HW) * sizeof(float) : 0; }
extern "C" int innfer_group_norm_skip(const void* d_u, int64_t u_gs, const void* d_skip, int64_t skip_gs, void* d_out, int64_t out_gs, int N, int64_t HW, int groups,
                                      const float* h_gamma, const float* h_beta, float eps, void* d_work, size_t work_bytes, void* stream) {
    if (!d_u || !d_skip || !d_out || !d_work || N <= 0 || N > 65535 || HW <= 0) return set_error(INNFER_ERR_INVALID, "group_norm_skip: null argument or N=%d HW=%lld", N, (long long)HW);
    if (groups != 1 && groups != 2 && groups != 4 && groups != 8) return set_error(INNFER_ERR_UNSUPPORTED, "group_norm_skip: %d groups of 64 channels (built: 1, 2, 4, 8)", groups);
    const int64_t G = (int64_t)N * HW * 32;
    if (u_gs < G || skip_gs < G || out_gs < G) return set_error(INNFER_ERR_INVALID, "group_norm_skip: a group stride below N * HW * 32");
    if (work_bytes < gn_work_floats(N, (long)HW) * sizeof(float)) return set_error(INNFER_ERR_WORKSPACE, "group_norm_skip: work_bytes %zu < %zu", work_bytes, gn_work_floats(N, (long)HW) * sizeof(float));
    float h[128];
    for (int i = 0; i < 64; ++i) { h[i] = h_gamma ? h_gamma[i] : 1.f; h[64 + i] = h_beta ? h_beta[i] : 0.f; }
    float* d_gn = nullptr;
    if (hipMalloc((void**)&d_gn, sizeof h) != hipSuccess) return set_error(INNFER_ERR_NOMEM, "group_norm_skip: out of device memory");
    int rc = hipMemcpy(d_gn, h, sizeof h, hipMemcpyHostToDevice) == hipSuccess ? INNFER_OK : set_error(INNFER_ERR_HIP, "group_norm_skip: copying the parameters failed");
    hipStream_t s = (hipStream_t)stream;
    if (rc == INNFER_OK) rc = gn_stats_launch((const f16*)d_u, (long)u_gs, N, (long)HW, (float*)d_work, s);
    if (rc == INNFER_OK) rc = gn_finalize_launch(N, (long)HW, groups, d_gn, d_gn + 64, eps, (float*)d_work, s);
    if (rc == INNFER_OK) rc = gn_apply_launch((const f16*)d_u, (long)u_gs, (const f16*)d_skip, (long)skip_gs, (f16*)d_out, (long)out_gs, N, (long)HW, (const float*)d_work, s);
    if (hipStreamSynchronize(s) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "group_norm_skip: a launch failed");
    (void)hipFree(d_gn);
    return rc;
}

// PixelShuffle(scale) of a conv slab + the nearest-upsampled input, as a single launch (for tests; SRVGGNetCompact's tail, csrc/shuffle_add.hip)
extern "C" int innfer_shuffle_add(const void* d_slab, int64_t group_stride, const void* d_base, int base_dtype, int normalize, void* d_out, int out_dtype,
                                  int N, int C, int H, int W, int scale, void* stream) {
    if ((d_base && base_dtype != INNFER_F16 && base_dtype != INNFER_U8) || (out_dtype != INNFER_F16 && out_dtype != INNFER_F32 && out_dtype != INNFER_U8))
        return set_error(INNFER_ERR_UNSUPPORTED, "shuffle_add: base fp16 or uint8, result fp16, fp32 or uint8");
    ShuffleAddLaunch T{};
    T.slab = (const f16*)d_slab; T.gstride = group_stride;
    T.base = d_base; T.base_u8 = base_dtype == INNFER_U8; T.base_norm = normalize != 0;
    T.out = d_out; T.out_mode = out_dtype == INNFER_U8 ? 2 : out_dtype == INNFER_F32 ? 1 : 0; T.out_denorm = normalize != 0;
    T.C = C; T.s = scale; T.N = N; T.H = H; T.W = W;
    return shuffle_add_launch(T, (hipStream_t)stream);
}

static int conv3x3_f16_impl(const innfer_conv_args* a, const float* d_slope, void* stream, int consumer_grid) {
    if (!a || !a->d_in || !a->d_packed || !a->d_bias || !a->d_out) return set_error(INNFER_ERR_INVALID, "conv3x3: null argument");
    // (121) the fields that reach the remaining forms of the kernel: mapped onto ConvLaunch below, conv_launch decides what is built
    const bool forms121 = a->conv1x1 || a->prefix_lrelu || a->d_gate_packed || a->d_gate_bias || a->in_relu || a->conv7x7 || a->out_planar || a->out_denorm || a->out_round16 ||
                          a->planar_phases || a->outm;
    if (forms121 && (a->column7 || a->stride2_k4 || a->transposed2x || a->pixel_shuffle2 || a->dilation > 1 || a->dilation_groups || a->d_stats_part))
        return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3: conv1x1 / prefix_lrelu / the self gate / in_relu / conv7x7 / out_planar / planar_phases / outm do not combine with "
                                                 "column7 / stride2_k4 / transposed2x / pixel_shuffle2 / dilation / d_stats_part");
    if ((a->act == 3 || a->act == 6) && !a->out_planar) return set_error(INNFER_ERR_INVALID, "conv3x3: act %d (tanh / sigmoid) is an activation of planar outputs (out_planar)", a->act);
    if (a->out_planar < 0 || a->out_planar > 3 || (!a->out_planar && (a->out_denorm || a->out_round16 || a->planar_phases)) || ((a->out_denorm || a->out_round16) && a->out_planar != 3))
        return set_error(INNFER_ERR_INVALID, "conv3x3: out_planar=%d (0..3); planar_phases needs out_planar, out_denorm / out_round16 the uint8 image (3)", a->out_planar);
    if (a->prefix_lrelu && !a->conv1x1) return set_error(INNFER_ERR_INVALID, "conv3x3: prefix_lrelu is an operand form of conv1x1");
    if ((a->d_gate_packed != nullptr) != (a->d_gate_bias != nullptr)) return set_error(INNFER_ERR_INVALID, "conv3x3: the self gate takes d_gate_packed and d_gate_bias");
    if (a->conv7x7 && !a->out_planar) return set_error(INNFER_ERR_UNSUPPORTED, "conv7x7: planar output (out_planar) with K <= 16 only");
    if (a->column7) {
        if (a->K <= 0 || a->K % 32 || a->K > 64 || a->out_ch_off || a->row_begin || a->row_end || a->dilation > 1 || a->dilation_groups || a->pixel_shuffle2 ||
            a->upsample2x || a->d_res1 || a->d_res2 || a->stride2_k4 || a->transposed2x || a->act < 0 || a->act > 2)
            return set_error(INNFER_ERR_UNSUPPORTED, "conv7x1: K %% 32 == 0, K <= 64 (K=%d), act 0..2, all rows, no residual / upsampling", a->K);
        ConvLaunch L{};
        L.in = (const f16*)a->d_in; L.in_gstride = a->in_group_stride; L.C = a->C;
        L.wpk = (const f16*)a->d_packed; L.bias = a->d_bias;
        L.out = a->d_out; L.out_gstride = a->out_group_stride; L.K = a->K;
        L.N = a->N; L.H = a->H; L.W = a->W; L.act = a->act; L.s1 = L.s2 = 1.f; L.y0 = 0; L.y1 = a->H; L.out_mode = OUT_SLAB;
        L.conv7v = 1; L.reflect = a->reflect_pad ? 1 : 0;
        if (int rc = conv_args_stats(a, 1, L)) return rc;
        return conv_launch(L, (hipStream_t)stream);
    }
    if (a->stride2_k4 || a->transposed2x) {
        if ((a->stride2_k4 && a->transposed2x) || (a->transposed2x && a->transposed2x != 3 && a->transposed2x != 4) || a->K <= 0 || a->K % 64 || a->out_ch_off ||
            a->row_begin || a->row_end || a->dilation > 1 || a->dilation_groups || a->reflect_pad || a->pixel_shuffle2 || a->upsample2x || a->d_res1 || a->d_res2 ||
            a->act < 0 || a->act > 2)
            return set_error(INNFER_ERR_UNSUPPORTED, "conv: the stride-2 forms need K %% 64 == 0 (K=%d), act 0..2, all rows, zero padding, no residual / upsampling", a->K);
        ConvLaunch L{};
        L.in = (const f16*)a->d_in; L.in_gstride = a->in_group_stride; L.C = a->C;
        L.wpk = (const f16*)a->d_packed; L.bias = a->d_bias;
        L.out = a->d_out; L.out_gstride = a->out_group_stride; L.K = a->K;
        L.N = a->N; L.H = a->H; L.W = a->W; L.act = a->act; L.s1 = L.s2 = 1.f; L.y0 = 0; L.y1 = a->H; L.out_mode = OUT_SLAB;
        if (a->stride2_k4) L.stride2 = 1;
        else { L.K = 4 * a->K; L.phase_c = a->K; L.deconv_phases = 1; L.rowp = a->plane_rows ? 1 : 0; }
        if (int rc = conv_args_stats(a, a->stride2_k4 ? 1 : 4, L)) return rc;
        return conv_launch(L, (hipStream_t)stream);
    }
    const int Kl = a->planar_phases ? 4 * a->K : a->K;           // planar_phases: the launch's channels are the four phases of K
    if (a->out_planar) {
        if (a->K <= 0 || a->K > 64 || Kl > 64 || a->out_ch_off)
            return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3: a planar output holds 1 .. 64 channels (K=%d%s) at out_ch_off 0", a->K, a->planar_phases ? ", four phases each" : "");
    } else if (a->pixel_shuffle2) {
        if (a->K <= 0 || a->K % 64 || a->out_ch_off || a->row_begin || a->row_end || a->dilation > 1 || a->dilation_groups || a->reflect_pad || a->act < 0 || a->act > 2)
            return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3: the PixelShuffle(2) store needs K %% 64 == 0 (K=%d), out_ch_off 0, act 0..2, all rows, plain zero padding", a->K);
    } else if (a->dilation_groups > 0 ? a->K != 32 * a->dilation_groups : (a->K <= 0 || a->K % 16 || (a->K > 64 && !(a->d_stats_part && a->K % 64 == 0))))
        return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3: K=%d (need K %% 16 == 0, K <= 64 -- with d_stats_part any K %% 64 == 0; K = 32 * dilation_groups)", a->K);
    ConvLaunch L{};
    if (a->out_ch_off % 16 || (a->out_ch_off % 32 && a->K > 16))
        return set_error(INNFER_ERR_INVALID, "conv3x3: out_ch_off=%d must keep the %d output channels inside 32-channel groups", a->out_ch_off, a->K);
    L.in = (const f16*)a->d_in; L.in_gstride = a->in_group_stride; L.C = a->C;
    L.wpk = (const f16*)a->d_packed; L.bias = a->d_bias;
    L.out = (f16*)a->d_out + (long)(a->out_ch_off / 32) * a->out_group_stride; L.out_gstride = a->out_group_stride;
    L.out_coff = a->out_ch_off % 32; L.K = a->K;
    L.N = a->N; L.H = a->H; L.W = a->W; L.act = a->act; L.up = a->upsample2x;
    L.res1 = (const f16*)a->d_res1; L.res1_gstride = a->res1_group_stride; L.s1 = a->res1_scale;
    L.res2 = (const f16*)a->d_res2; L.res2_gstride = a->res2_group_stride; L.s2 = a->res2_scale;
    L.y0 = a->row_begin; L.y1 = a->row_end > 0 ? a->row_end : a->H;
    L.out_mode = a->pixel_shuffle2 ? OUT_SHUFFLE2 : OUT_SLAB; L.reflect = a->reflect_pad; L.dilation = a->dilation; L.dilation_groups = a->dilation_groups;
    L.res1_lds = a->res1_from_input ? 2 : 0;                 // (the single-conv call: wherever the shape qualifies, one residual or two)
    L.slope = d_slope;
    L.grid2 = consumer_grid;
    L.rowp = a->plane_rows ? 1 : 0;
    if (a->pixel_shuffle2 && a->plane_rows == 2) L.rowp = 2;          // phase-major panels + bias from innfer_pack_conv3x3_shuffle2: the producer / consumer kernel's store
    else if (a->pixel_shuffle2 && a->plane_rows) return set_error(INNFER_ERR_INVALID, "conv3x3: pixel_shuffle2 takes plane_rows 0 (innfer_pack_conv3x3 panels) or 2 (innfer_pack_conv3x3_shuffle2 panels)");
    if (a->reserved0) return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3: innfer_conv_args.reserved0 (the row-Winograd experiment until ABI 111) must be 0");
    L.conv1x1 = a->conv1x1 ? 1 : 0; L.prefix_lrelu = a->prefix_lrelu ? 1 : 0; L.in_relu = a->in_relu ? 1 : 0; L.conv7 = a->conv7x7 ? 1 : 0;
    L.gate_w = (const f16*)a->d_gate_packed; L.gate_bias = a->d_gate_bias;
    L.outm = a->outm;
    if (a->out_planar) {               // d_out is the planar tensor / the uint8 image
        L.out = a->d_out; L.out_coff = 0; L.K = Kl; L.out_mode = OUT_NCHW;
        L.out_f32 = a->out_planar == 2; L.out_u8 = a->out_planar == 3; L.out_denorm = a->out_denorm ? 1 : 0; L.out_round16 = a->out_round16 ? 1 : 0;
        L.phase_c = a->planar_phases ? a->K : 0;
    }
    if (a->split) {
        if (a->pixel_shuffle2 || (!a->out_planar && (a->K % 32 || a->out_lo <= 0)) || a->in_lo <= 0 || (a->d_res1 && a->res1_lo <= 0) || (a->d_res2 && a->res2_lo <= 0))
            return set_error(INNFER_ERR_UNSUPPORTED, "conv3x3 (split): K in {32, 64} (K=%d), slab output, the lo distances of every tensor given", a->K);
        L.split = 1; L.in_lo = a->in_lo; L.out_lo = a->out_lo; L.res1_lo = a->res1_lo; L.res2_lo = a->res2_lo;
    }
    if (int rc = conv_args_stats(a, 1, L)) return rc;
    return conv_launch(L, (hipStream_t)stream);
}

extern "C" int innfer_nchw_to_slab(const void* d_src, int src_dtype, void* d_slab, int64_t group_stride, int ch_off,
                                   int N, int C, int H, int W, void* stream) {
    return nchw_to_slab(d_src, src_dtype == INNFER_F32, (f16*)d_slab, group_stride, ch_off, N, C, H, W, (hipStream_t)stream);
}

extern "C" int innfer_slab_to_nchw(const void* d_slab, int64_t group_stride, int ch_off, void* d_dst, int dst_dtype,
                                   int N, int C, int H, int W, void* stream) {
    return slab_to_nchw((const f16*)d_slab, group_stride, ch_off, d_dst, dst_dtype == INNFER_F32, N, C, H, W, (hipStream_t)stream);
}

// conv3x3(pixel_unshuffle(x, r)) alone, for tests: packs and uploads the weights, launches conv_first_unshuffle.hip's kernel into a slab on the LR grid, waits.
extern "C" int innfer_first_conv_unshuffle(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W, int unshuffle,
                                           const float* h_weight_oihw, const float* h_bias, int K, int act, void* d_slab, int64_t group_stride, int64_t lo, void* stream) {
    if (!d_in || !h_weight_oihw || !d_slab) return set_error(INNFER_ERR_INVALID, "first_conv_unshuffle: null argument");
    if (in_dtype != INNFER_F16 && in_dtype != INNFER_F32 && in_dtype != INNFER_U8) return set_error(INNFER_ERR_INVALID, "first_conv_unshuffle: bad dtype");
    if ((unshuffle != 2 && unshuffle != 4) || in_nc != 3 || (K != 32 && K != 64) || act < 0 || act > 2 || N <= 0 || H <= 0 || W <= 0)
        return set_error(INNFER_ERR_UNSUPPORTED, "first_conv_unshuffle: unshuffle %d (2 | 4), in_nc %d (3), K %d (32 | 64), act %d (0..2)", unshuffle, in_nc, K, act);
    const long px = (long)N * ((H + unshuffle - 1) / unshuffle) * ((W + unshuffle - 1) / unshuffle);
    if (group_stride < px * 32 || lo < 0) return set_error(INNFER_ERR_INVALID, "first_conv_unshuffle: group_stride %ld < %ld", (long)group_stride, px * 32);
    std::vector<char> host(first_unshuffle_packed_bytes(K, unshuffle));
    first_unshuffle_pack(h_weight_oihw, K, unshuffle, host.data());
    std::vector<float> bias(K, 0.f);
    if (h_bias) for (int k = 0; k < K; ++k) bias[k] = h_bias[k];
    void* d_w = nullptr; float* d_b = nullptr;
    INNFER_HIP(hipMalloc(&d_w, host.size()));
    if (hipMalloc((void**)&d_b, K * sizeof(float)) != hipSuccess) { (void)hipFree(d_w); return set_error(INNFER_ERR_NOMEM, "first_conv_unshuffle: out of device memory"); }
    int rc = INNFER_OK;
    if (hipMemcpy(d_w, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_b, bias.data(), K * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        rc = set_error(INNFER_ERR_HIP, "first_conv_unshuffle: copying the weights failed");
    if (rc == INNFER_OK) {
        FirstUnshuffleLaunch F{};
        F.in = d_in; F.in_f32 = in_dtype == INNFER_F32; F.Cin = in_nc; F.in_u8 = in_dtype == INNFER_U8; F.in_norm = normalize != 0; F.in_round16 = fp16_mode != 0;
        F.r = unshuffle; F.wpk = d_w; F.bias = d_b; F.out = (f16*)d_slab; F.out_gstride = group_stride; F.K = K; F.N = N; F.H = H; F.W = W; F.act = act; F.out_lo = lo;
        rc = first_unshuffle_launch(F, (hipStream_t)stream);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "first_conv_unshuffle: the launch failed");
    }
    (void)hipFree(d_w); (void)hipFree(d_b);
    return rc;
}

// The first conv of RRDBNet / SRResNet / SRVGGNetCompact (and PPON) alone, for tests: first_conv_layout + first_conv_launch, the code the networks run.  Uploads, launches, waits.
static int first_conv_impl(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                           const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_slope, const float* h_alpha, const float* h_shift,
                           void* d_slab, int64_t group_stride, int64_t lo, void* d_slab2, int64_t group_stride2, int64_t lo2, void* stream);
extern "C" int innfer_first_conv(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                                 const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_slope,
                                 void* d_slab, int64_t group_stride, int64_t lo, void* d_slab2, int64_t group_stride2, int64_t lo2, void* stream) {
    return first_conv_impl(d_in, in_dtype, normalize, fp16_mode, N, in_nc, H, W, h_weight_oihw, h_bias, K, act, h_slope, nullptr, nullptr, d_slab, group_stride, lo, d_slab2, group_stride2, lo2, stream);
}
// The same launch with the per-input-channel map in front of the conv (FirstConvLaunch.in_map; SPAN's conv_1): operand = fp16(h_alpha[c] * v + h_shift[c]); either
// vector NULL means 1 / 0, both NULL no map at all (innfer_first_conv's launch).
extern "C" int innfer_first_conv_map(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                                     const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_alpha, const float* h_shift,
                                     void* d_slab, int64_t group_stride, void* stream) {
    return first_conv_impl(d_in, in_dtype, normalize, fp16_mode, N, in_nc, H, W, h_weight_oihw, h_bias, K, act, nullptr, h_alpha, h_shift, d_slab, group_stride, 0, nullptr, 0, 0, stream);
}
static int first_conv_impl(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                           const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_slope, const float* h_alpha, const float* h_shift,
                           void* d_slab, int64_t group_stride, int64_t lo, void* d_slab2, int64_t group_stride2, int64_t lo2, void* stream) {
    if (!d_in || !h_weight_oihw || !d_slab) return set_error(INNFER_ERR_INVALID, "first_conv: null argument");
    if (in_dtype != INNFER_F16 && in_dtype != INNFER_F32 && in_dtype != INNFER_U8) return set_error(INNFER_ERR_INVALID, "first_conv: bad dtype");
    if ((K != 32 && K != 64) || in_nc < 1 || in_nc > 8 || (act != 0 && act != 1 && act != 2 && act != 8))
        return set_error(INNFER_ERR_UNSUPPORTED, "first_conv: K %d (32 | 64), in_nc %d (1..8), act %d (0, 1, 2, 8)", K, in_nc, act);
    if (N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "first_conv: bad shape %dx%dx%d", N, H, W);
    const long px = (long)N * H * W, need_lo = (long)(K / 32 - 1);
    if (group_stride < px * 32 || (d_slab2 && group_stride2 < px * 32))
        return set_error(INNFER_ERR_INVALID, "first_conv: group stride %ld / %ld < %ld", (long)group_stride, (long)group_stride2, px * 32);
    if (lo < 0 || lo2 < 0 || (lo && lo < need_lo * group_stride + px * 32) || (d_slab2 && ((lo != 0) != (lo2 != 0) || (lo2 && lo2 < need_lo * group_stride2 + px * 32))) || (!d_slab2 && lo2))
        return set_error(INNFER_ERR_INVALID, "first_conv: the lo distances (%ld, %ld) must be 0 or clear the hi slab, and be given for both slabs or neither", (long)lo, (long)lo2);
    if (act == 8 && !h_slope) return set_error(INNFER_ERR_INVALID, "first_conv: act 8 needs the slope vector");
    if (act == 8 && (lo || lo2)) return set_error(INNFER_ERR_UNSUPPORTED, "first_conv: act 8 is built for fp16 outputs (no split output)");
    std::vector<float> host((size_t)in_nc * 9 * K), bias(K, 0.f);
    first_conv_layout(h_weight_oihw, K, in_nc, host.data());
    if (h_bias) for (int k = 0; k < K; ++k) bias[k] = h_bias[k];
    float *d_w = nullptr, *d_b = nullptr, *d_s = nullptr, *d_m = nullptr;
    int rc = INNFER_OK;
    const bool mapped = h_alpha || h_shift;
    float h_map[16];
    for (int c = 0; c < in_nc; ++c) { h_map[c] = h_alpha ? h_alpha[c] : 1.f; h_map[in_nc + c] = h_shift ? h_shift[c] : 0.f; }
    if (hipMalloc((void**)&d_w, host.size() * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_b, K * sizeof(float)) != hipSuccess ||
        (act == 8 && hipMalloc((void**)&d_s, K * sizeof(float)) != hipSuccess) || (mapped && hipMalloc((void**)&d_m, 2 * in_nc * sizeof(float)) != hipSuccess))
        rc = set_error(INNFER_ERR_NOMEM, "first_conv: out of device memory");
    if (rc == INNFER_OK && d_m && hipMemcpy(d_m, h_map, 2 * in_nc * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = set_error(INNFER_ERR_HIP, "first_conv: copying the input map failed");
    if (rc == INNFER_OK && (hipMemcpy(d_w, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
                            hipMemcpy(d_b, bias.data(), K * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
                            (d_s && hipMemcpy(d_s, h_slope, K * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)))
        rc = set_error(INNFER_ERR_HIP, "first_conv: copying the weights failed");
    if (rc == INNFER_OK) {
        FirstConvLaunch F{};
        F.in = d_in; F.in_f32 = in_dtype == INNFER_F32; F.Cin = in_nc; F.in_u8 = in_dtype == INNFER_U8; F.in_norm = normalize != 0; F.in_round16 = fp16_mode != 0;
        F.w = d_w; F.bias = d_b; F.out = (f16*)d_slab; F.out_gstride = group_stride; F.out2 = (f16*)d_slab2; F.out2_gstride = group_stride2;
        F.K = K; F.N = N; F.H = H; F.W = W; F.act = act; F.out_lo = lo; F.out2_lo = lo2; F.slope = d_s; F.in_map = d_m;
        rc = first_conv_launch(F, (hipStream_t)stream);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "first_conv: the launch failed");
    }
    (void)hipFree(d_w); (void)hipFree(d_b); (void)hipFree(d_s); (void)hipFree(d_m);
    return rc;
}

// The slab passes of innfer_net_forward as single launches, for tests: each checks its arguments and calls the launcher the network calls.
static int slab_pass_args(const char* what, const void* a, const void* b, int N, int H, int W, int f, int64_t src_gs, int64_t dst_gs, int64_t lo, long src_need, long dst_need) {
    if (!a || !b) return set_error(INNFER_ERR_INVALID, "%s: null argument", what);
    if (N <= 0 || H <= 0 || W <= 0 || f < 1) return set_error(INNFER_ERR_INVALID, "%s: bad shape %dx%dx%d, factor %d", what, N, H, W, f);
    if ((long)H * f > 32768 || (long)W * f > 32768 || (long)N * H * f * W * f > (1L << 30)) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d images of %d x %d at factor %d", what, N, H, W, f);
    const long px = (long)N * H * W;
    if (src_gs < px * 32 || dst_gs < px * f * f * 32) return set_error(INNFER_ERR_INVALID, "%s: group strides %ld / %ld < %ld / %ld", what, (long)src_gs, (long)dst_gs, px * 32, px * f * f * 32);
    if (lo < 0 || (lo && (lo < src_need || lo < dst_need))) return set_error(INNFER_ERR_INVALID, "%s: lo %ld must be 0 or clear both hi slabs", what, (long)lo);
    return INNFER_OK;
}

extern "C" int innfer_slab_upsample_nearest(const void* d_src, int64_t src_gs, void* d_dst, int64_t dst_gs, int groups, int N, int H, int W, int factor, int64_t lo, void* stream) {
    if (groups < 1 || groups > 64) return set_error(INNFER_ERR_INVALID, "slab_upsample_nearest: %d groups", groups);
    const long px = (long)N * H * W;
    if (int rc = slab_pass_args("slab_upsample_nearest", d_src, d_dst, N, H, W, factor, src_gs, dst_gs, lo, (groups - 1) * src_gs + px * 32, (groups - 1) * dst_gs + px * factor * factor * 32)) return rc;
    return launch_upsample_nearest((const f16*)d_src, src_gs, (f16*)d_dst, dst_gs, groups, N, H, W, factor, (hipStream_t)stream, lo);
}

extern "C" int innfer_slab_pixel_shuffle(const void* d_src, int64_t src_gs, void* d_dst, int64_t dst_gs, int nf, int N, int H, int W, int r, int64_t lo, void* stream) {
    if (nf < 8 || nf % 8 || nf > 2048) return set_error(INNFER_ERR_INVALID, "slab_pixel_shuffle: nf %d must be a positive multiple of 8", nf);
    if (r < 1 || r > 8) return set_error(INNFER_ERR_INVALID, "slab_pixel_shuffle: factor %d", r);
    const long px = (long)N * H * W;
    if (int rc = slab_pass_args("slab_pixel_shuffle", d_src, d_dst, N, H, W, r, src_gs, dst_gs, lo, (long)((nf * r * r + 31) / 32 - 1) * src_gs + px * 32, (long)((nf + 31) / 32 - 1) * dst_gs + px * r * r * 32)) return rc;
    return launch_pixel_shuffle((const f16*)d_src, src_gs, (f16*)d_dst, dst_gs, nf, N, H, W, r, (hipStream_t)stream, lo);
}

// dst = act(alpha[c] * src + shift[c]) over every element of ceil(C / 32) groups of gs elements (channels beyond C: zero); lo != 0: on the (hi, lo) pairs.  Uploads the map, launches, waits.
extern "C" int innfer_slab_input_map(const void* d_src, void* d_dst, int64_t gs, int64_t lo, int C, const float* h_alpha, const float* h_shift, int act, void* stream) {
    if (!d_src || !d_dst) return set_error(INNFER_ERR_INVALID, "slab_input_map: null argument");
    if (C < 1 || C > 2048 || act < 0 || act > 2) return set_error(INNFER_ERR_INVALID, "slab_input_map: C %d, act %d (0..2)", C, act);
    if (gs < 32 || gs % 32 || gs > (1L << 31)) return set_error(INNFER_ERR_INVALID, "slab_input_map: a group of %ld elements (whole pixels of 32 channels)", (long)gs);
    const long groups = (C + 31) / 32;
    if (lo < 0 || (lo && lo < groups * gs)) return set_error(INNFER_ERR_INVALID, "slab_input_map: lo %ld must be 0 or clear the %ld groups of the hi slab", (long)lo, groups);
    std::vector<float> h(2 * (size_t)C);
    for (int i = 0; i < C; ++i) { h[i] = h_alpha ? h_alpha[i] : 1.f; h[C + i] = h_shift ? h_shift[i] : 0.f; }
    float* d_map = nullptr;
    if (hipMalloc((void**)&d_map, h.size() * sizeof(float)) != hipSuccess) return set_error(INNFER_ERR_NOMEM, "slab_input_map: out of device memory");
    int rc = INNFER_OK;
    if (hipMemcpy(d_map, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = set_error(INNFER_ERR_HIP, "slab_input_map: copying the map failed");
    if (rc == INNFER_OK) {
        rc = launch_input_map((const f16*)d_src, (f16*)d_dst, gs, C, d_map, act, (hipStream_t)stream, lo);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "slab_input_map: the launch failed");
    }
    (void)hipFree(d_map);
    return rc;
}
