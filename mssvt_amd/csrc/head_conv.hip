// head_conv.hip -- CenterHead's eleven 3x3 convolutions in eval mode as three launches on channels-last fp32 tensors (ref
// pcdet/models/dense_heads/center_head.py: shared_conv :76-84, SeparateHead :11-46, forward :350-360), on the split-fp16
// v_mfma_f32_16x16x32_f16 kernel of split_conv.hip.h, which holds the arithmetic, the pipeline and the blob layout.  What is
// this file's own: the mssvt_head_conv_* entry points and the three stages, all k_split_conv with the 3x3 / stride 1 taps
// folded, sliced input and one header record per slice (its own weight power of two, k and kbase):
//   shared  3x3 Cin -> S + BN + ReLU:            1 slice, reads all Cin channels (Cin in {64, 256, 384, 512}, S in {32, 64}),
//                                                 writes (B, H, W, S) and one exponent word per pixel (the largest |y| of the
//                                                 pixel, from the epilogue);
//   trunk   3x3 S -> nb S + BN + ReLU:           nb <= 64 slices (the first convolution of every branch of every head), all
//                                                 read the same S channels, slice b writes columns [b S, (b + 1) S) of
//                                                 (B, H, W, nb S) and exponent word [pixel][b]: ONE WORD PER PIXEL AND
//                                                 BRANCH, so that a branch whose BatchNorm leaves it many binades below
//                                                 another keeps its own normalisation in the next stage;
//   finals  3x3 S -> k_b + bias, no activation:  nb slices of one 16-column tile, slice b reads only channels
//                                                 [b S, (b + 1) S) of the trunk tensor under its own exponent words and
//                                                 writes its k_b <= 16 maps PLANAR: y[kbase_b B H W + (b' k_b + c) H W + r]
//                                                 for sample b', map c, cell r.
// The trunk and the finals are packed one branch (slice) per call.  (Reading a small slice's nine taps into LDS once instead
// of streaming them was measured on the finals at 470 x 470: 2 % slower, so there is one form.)
#include "split_conv.hip.h"

#define HC_MAX_SLICES 64

static bool hc_cin(int cin) { return cin == 64 || cin == 256 || cin == 384 || cin == 512; }
static bool hc_s(int s) { return s == 32 || s == 64; }

extern "C" int mssvt_head_conv_supported(int cin, int s, int nb, int kmax) {
    return hc_cin(cin) && hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES && kmax >= 1 && kmax <= 16 ? 1 : 0;
}

static long long hc_bytes(int cin, int ns, int nsl) { return BC_HDR(nsl) + 8ll * nsl * ns + 36ll * cin * nsl * ns; }

extern "C" long long mssvt_head_conv_shared_pack_bytes(int cin, int s) {
    return hc_cin(cin) && hc_s(s) ? hc_bytes(cin, s, 1) : 0;
}
extern "C" long long mssvt_head_conv_trunk_pack_bytes(int s, int nb) {
    return hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES ? hc_bytes(s, s, nb) : 0;
}
extern "C" long long mssvt_head_conv_finals_pack_bytes(int s, int nb) {
    return hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES ? hc_bytes(s, 16, nb) : 0;
}

// slice sl of nsl: a (k, cin, 3, 3) weight into ns >= k columns
static int hc_pack_slice(const float *w, const float *bias, const float *bn_w, const float *bn_b, const float *bn_mean,
                         const float *bn_var, float eps, int cin, int k, int kbase, int ns, int nsl, int sl, void *packed,
                         void *stream) {
    return bc_pack(w, 0, bias, bn_w, bn_b, bn_mean, bn_var, eps, 3, cin, k, kbase, ns, nsl, sl, 0, packed, (hipStream_t)stream);
}

extern "C" int mssvt_head_conv_shared_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                           const float *bn_mean, const float *bn_var, float bn_eps, int cin, int s, void *packed,
                                           void *stream) {
    if (!weight || !packed || cin <= 0 || s <= 0 || bc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s)) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, cin, s, 0, s, 1, 0, packed, stream);
}

extern "C" int mssvt_head_conv_trunk_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                          const float *bn_mean, const float *bn_var, float bn_eps, int s, int nb, int branch,
                                          void *packed, void *stream) {
    if (!weight || !packed || s <= 0 || nb <= 0 || branch < 0 || branch >= nb ||
        bc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, s, s, 0, s, nb, branch, packed, stream);
}

extern "C" int mssvt_head_conv_finals_pack(const float *weight, const float *bias, int s, int nb, int branch, int k, int kbase,
                                           void *packed, void *stream) {
    if (!weight || !packed || s <= 0 || nb <= 0 || branch < 0 || branch >= nb || k <= 0 || kbase < 0 || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || k > 16 || kbase > 16 * HC_MAX_SLICES) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, nullptr, nullptr, nullptr, nullptr, 0.f, s, k, kbase, 16, nb, branch, packed, stream);
}

static int hc_expmap(const float *x, long long rows, int c, int *emap, hipStream_t st) {
#define HC_EXP(C) \
    if (c == C) return bc_expmap<C, (C / 4 < 16 ? C / 4 : 16)>(x, rows, emap, st);
    HC_EXP(32) HC_EXP(64) HC_EXP(256) HC_EXP(384) HC_EXP(512)
#undef HC_EXP
    return MSSVT_E_TOOLARGE;
}

// x (rows, c) f32 -> exp_words (rows) int32: the largest |x| of every row as bits (what the stages' exp_out hold)
extern "C" int mssvt_head_conv_expmap(const float *x, long long rows, int c, int *exp_words, void *stream) {
    if (!x || !exp_words || rows <= 0 || c <= 0 || bc_misaligned(x)) return MSSVT_E_BADARG;
    if (!(hc_cin(c) || hc_s(c)) || rows > 0x7FFFFFFFll * 16) return MSSVT_E_TOOLARGE;
    return hc_expmap(x, rows, c, exp_words, (hipStream_t)stream);
}

// x: pixels of `xstride` floats, slice sl reads channels [sl gin, sl gin + CIN) and word sl of emap [pixel][egroups] (word 0
// when egroups == 1)
template <int CIN, int NS, int OUT>
static int hc_launch(const float *x, int xstride, int gin, int B, int H, int W, const void *packed, int nsl, const int *emap,
                     int egroups, int relu, float *y, int *eout, void *stream) {
    return bc_launch<CIN, NS, 3, true, OUT>(x, xstride, gin, H, W, H, W, B * H * W, packed, nsl, 3, 1, 1, emap, egroups, relu, y,
                                            eout, 0, 0, (hipStream_t)stream);
}

// x (B, H, W, cin) -> y (B, H, W, s) = relu(scale conv + shift); exp_workspace (B H W) int32 written here (the input's
// exponent words); exp_out (B H W) int32: y's exponent words, for the trunk
extern "C" int mssvt_head_conv_shared(const float *x, int B, int H, int W, int cin, int s, const void *packed, int *exp_workspace,
                                      float *y, int *exp_out, void *stream) {
    if (!x || !packed || !exp_workspace || !y || !exp_out || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || s <= 0 ||
        bc_misaligned(x) || bc_misaligned(y) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    int status = hc_expmap(x, (long long)B * H * W, cin, exp_workspace, (hipStream_t)stream);
    if (status != MSSVT_OK) return status;
#define HC_GO(CI, S) \
    if (cin == CI && s == S)  \
        return hc_launch<CI, S, BC_ROWS_WORDS>(x, CI, 0, B, H, W, packed, 1, exp_workspace, 1, 1, y, exp_out, stream);
    HC_GO(64, 32) HC_GO(64, 64) HC_GO(256, 32) HC_GO(256, 64) HC_GO(384, 32) HC_GO(384, 64) HC_GO(512, 32) HC_GO(512, 64)
#undef HC_GO
    return MSSVT_E_TOOLARGE;
}

// x (B, H, W, s) with its exponent words exp_in (B H W) -> y (B, H, W, nb s), exp_out (B H W, nb): one word per pixel and branch
extern "C" int mssvt_head_conv_trunk(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                                     float *y, int *exp_out, void *stream) {
    if (!x || !packed || !exp_in || !y || !exp_out || B <= 0 || H <= 0 || W <= 0 || s <= 0 || nb <= 0 || bc_misaligned(x) ||
        bc_misaligned(y) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    if (s == 32) return hc_launch<32, 32, BC_ROWS_WORDS>(x, 32, 0, B, H, W, packed, nb, exp_in, 1, 1, y, exp_out, stream);
    return hc_launch<64, 64, BC_ROWS_WORDS>(x, 64, 0, B, H, W, packed, nb, exp_in, 1, 1, y, exp_out, stream);
}

// x (B, H, W, nb s) with exp_in (B H W, nb) -> y planar: branch b's (B, k_b, H, W) maps start at float kbase_b B H W
extern "C" int mssvt_head_conv_finals(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                                      float *y, void *stream) {
    if (!x || !packed || !exp_in || !y || B <= 0 || H <= 0 || W <= 0 || s <= 0 || nb <= 0 || bc_misaligned(x) ||
        bc_misaligned(y) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    if (s == 32) return hc_launch<32, 16, BC_PLANAR>(x, nb * 32, 32, B, H, W, packed, nb, exp_in, nb, 0, y, nullptr, stream);
    return hc_launch<64, 16, BC_PLANAR>(x, nb * 64, 64, B, H, W, packed, nb, exp_in, nb, 0, y, nullptr, stream);
}
