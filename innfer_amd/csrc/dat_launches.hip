// The single-launch C entries of DAT's kernels (for tests; include/innfer_amd.h documents each), on test_entry.h's Upload and finish.
#include "test_entry.h"

using namespace innfer;

extern "C" int innfer_window_attention_rect(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int H, int W, int num_heads,
                                            int head_dim, int s0, int s1, int shifted, void* stream) {
    if (!d_qkv || !d_out || !h_bias) return set_error(INNFER_ERR_INVALID, "window_attention_rect: null argument");
    if (s0 != 8 || (s1 != 32 && s1 != 16)) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention_rect: split [%d, %d] (built: [8, 32] and [8, 16])", s0, s1);
    if (num_heads < 2 || num_heads > 8 || (num_heads & 1)) return set_error(INNFER_ERR_UNSUPPORTED, "window_attention_rect: %d heads (built: 2, 4, 6, 8)", num_heads);
    const size_t T = (size_t)s0 * s1;
    Upload b("window_attention_rect", {{h_bias, (size_t)num_heads * T * T}});
    int rc = b.rc;
    if (rc == INNFER_OK) rc = win_attn_rect_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, b.d, N, H, W, num_heads, head_dim, s0, s1, shifted, (hipStream_t)stream);
    return finish("window_attention_rect", rc, stream);
}

extern "C" size_t innfer_channel_attention_work_bytes(int N, int64_t HW, int num_heads) {
    return (N > 0 && HW > 0 && num_heads > 0) ? csa_work_floats(N, (long)HW, num_heads) * sizeof(float) : 0;
}

extern "C" int innfer_channel_attention_scores(const void* d_qkv, int64_t qkv_gs, int N, int64_t HW, int num_heads, int head_dim, const float* h_temperature, void* d_A,
                                               void* d_gram, void* d_work, size_t work_bytes, void* stream) {
    if (!d_qkv || !h_temperature || !d_A || !d_work) return set_error(INNFER_ERR_INVALID, "channel_attention_scores: null argument");
    if (N <= 0 || HW <= 0) return set_error(INNFER_ERR_INVALID, "channel_attention_scores: N=%d HW=%lld", N, (long long)HW);
    if (num_heads < 1 || num_heads > 8 || head_dim < 1 || head_dim > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "channel_attention_scores: %d heads of %d channels (built: <= 8 heads, <= 32 channels)", num_heads, head_dim);
    if (work_bytes < innfer_channel_attention_work_bytes(N, HW, num_heads))
        return set_error(INNFER_ERR_WORKSPACE, "channel_attention_scores: work buffer %zu < %zu bytes", work_bytes, innfer_channel_attention_work_bytes(N, HW, num_heads));
    if (((uintptr_t)d_work | (uintptr_t)d_A) & 15) return set_error(INNFER_ERR_INVALID, "channel_attention_scores: d_work and d_A must be 16-byte aligned");
    Upload t("channel_attention_scores", {{h_temperature, (size_t)num_heads}});
    int rc = t.rc;
    if (rc == INNFER_OK) rc = csa_scores_launch((const f16*)d_qkv, (long)qkv_gs, N, (long)HW, num_heads, head_dim, t.d, (float*)d_work, (float*)d_A, (float*)d_gram, (hipStream_t)stream);
    return finish("channel_attention_scores", rc, stream);
}

extern "C" int innfer_channel_attention_apply(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const void* d_A, int N, int64_t HW, int num_heads, int head_dim,
                                              void* stream) {
    if (!d_qkv || !d_out || !d_A) return set_error(INNFER_ERR_INVALID, "channel_attention_apply: null argument");
    int rc = csa_apply_launch((const f16*)d_qkv, (long)qkv_gs, (f16*)d_out, (long)out_gs, (const float*)d_A, N, (long)HW, num_heads, head_dim, (hipStream_t)stream);
    return finish("channel_attention_apply", rc, stream);
}

extern "C" int innfer_dwconv3x3(const void* d_in, int64_t in_gs, const void* d_mul, int64_t mul_gs, void* d_out, int64_t out_gs, int N, int H, int W, int C, int c_pad,
                                const float* h_taps, const float* h_bias, int epilogue, void* stream) {
    if (!d_in || !d_out || !h_taps || !h_bias) return set_error(INNFER_ERR_INVALID, "dwconv3x3: null argument");
    if (C < 1 || C > 512) return set_error(INNFER_ERR_UNSUPPORTED, "dwconv3x3: C=%d (built: 1 .. 512)", C);
    Upload p("dwconv3x3", {{h_taps, (size_t)C * 9}, {h_bias, (size_t)C}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = dwconv3x3_launch((const f16*)d_in, (long)in_gs, (const f16*)d_mul, (long)mul_gs, (f16*)d_out, (long)out_gs, N, H, W, C, c_pad, p.d, p.d + (size_t)C * 9,
                                               epilogue, (hipStream_t)stream);
    return finish("dwconv3x3", rc, stream);
}

extern "C" int innfer_chan_attn_excite_gelu(const void* d_z, int64_t z_gs, int N, int64_t HW, int C, int c_pad, int hidden, const float* h_w1, const float* h_b1,
                                            const float* h_w2, const float* h_b2, void* d_y, void* d_sums, void* d_work, size_t work_bytes, void* stream) {
    if (!d_z || !h_w1 || !h_b1 || !h_w2 || !h_b2 || !d_y || !d_work) return set_error(INNFER_ERR_INVALID, "chan_attn_excite_gelu: null argument");
    if (N <= 0 || HW <= 0 || C < 1 || C > 256 || c_pad < C || c_pad > 256 || c_pad % 64 || hidden < 1 || hidden > 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "chan_attn_excite_gelu: N=%d HW=%ld C=%d c_pad=%d hidden=%d (built: C <= c_pad in 64, 128, 192, 256; hidden <= 64)", N, (long)HW, C, c_pad, hidden);
    if (work_bytes < innfer_chan_attn_work_bytes(N, HW, c_pad))
        return set_error(INNFER_ERR_WORKSPACE, "chan_attn_excite_gelu: work buffer %zu < %zu bytes", work_bytes, innfer_chan_attn_work_bytes(N, HW, c_pad));
    Upload p("chan_attn_excite_gelu", {{h_w1, (size_t)hidden * C}, {h_b1, (size_t)hidden}, {h_w2, (size_t)C * hidden}, {h_b2, (size_t)C}});
    int rc = p.rc;
    hipStream_t s = (hipStream_t)stream;
    if (rc == INNFER_OK) rc = ca_pool_launch((const f16*)d_z, (long)z_gs, N, (long)HW, c_pad, (float*)d_work, s);
    if (rc == INNFER_OK) rc = ca_excite_gelu_launch((const float*)d_work, N, (long)HW, C, c_pad, hidden, p.d, p.d + (size_t)hidden * C, p.d + (size_t)hidden * C + hidden,
                                                    p.d + 2 * (size_t)hidden * C + hidden, (float*)d_y, (float*)d_sums, s);
    return finish("chan_attn_excite_gelu", rc, stream);
}

extern "C" int innfer_aim_mix(const void* d_x, int64_t x_gs, const void* d_y, int64_t y_gs, void* d_out, int64_t out_gs, const void* d_gate, int N, int64_t HW, int C, int c_pad,
                              int hidden, const float* h_w1, const float* h_b1, const float* h_w2, float b2, void* stream) {
    if (!d_x || !d_y || !d_out || !d_gate || !h_w1 || !h_b1 || !h_w2) return set_error(INNFER_ERR_INVALID, "aim_mix: null argument");
    if (C < 1 || C > 256 || hidden < 1 || hidden > 16) return set_error(INNFER_ERR_UNSUPPORTED, "aim_mix: C=%d, %d hidden channels (built: C <= 256, hidden <= 16)", C, hidden);
    Upload p("aim_mix", {{h_w1, (size_t)hidden * C}, {h_b1, (size_t)hidden}, {h_w2, (size_t)hidden}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = aim_mix_launch((const f16*)d_x, (long)x_gs, (const f16*)d_y, (long)y_gs, (f16*)d_out, (long)out_gs, (const float*)d_gate, N, (long)HW, C, c_pad, hidden,
                                             p.d, p.d + (size_t)hidden * C, p.d + (size_t)hidden * C + hidden, b2, (hipStream_t)stream);
    return finish("aim_mix", rc, stream);
}

extern "C" int innfer_layer_norm_wide(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad, const float* h_gamma, const float* h_beta,
                                      float eps, void* stream) {
    if (!d_in || !d_out || !h_gamma || !h_beta) return set_error(INNFER_ERR_INVALID, "layer_norm_wide: null argument");
    if (C < 1 || C > 512) return set_error(INNFER_ERR_UNSUPPORTED, "layer_norm_wide: C=%d (built: 1 .. 512)", C);
    Upload p("layer_norm_wide", {{h_gamma, (size_t)C}, {h_beta, (size_t)C}});
    int rc = p.rc;
    if (rc == INNFER_OK) rc = layer_norm_wide_launch((const f16*)d_in, (long)in_gs, (f16*)d_out, (long)out_gs, (long)npix, C, c_pad, p.d, p.d + C, eps, (hipStream_t)stream);
    return finish("layer_norm_wide", rc, stream);
}
