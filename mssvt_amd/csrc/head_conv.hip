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
// The second half of the file is the TRAINING path of the shared layer and the trunk (forward without BatchNorm / ReLU, input,
// weight and bias gradients): see the comment at its head.
#include "split_conv.hip.h"
#include "split_wgrad.hip.h"

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

// ---- training: the shared layer and the trunk without BatchNorm / ReLU, forward and backward ---------------------------------------
// (ref center_head.py :76-84 and :11-46 in training mode: Conv2d 3x3 (+ bias) whose BatchNorm2d + ReLU stay modules.)
//   shared  y = conv(x, W) + bias: the inference kernel with scale 1, shift = bias, no ReLU, plain rows (BC_ROWS);
//           dX = the convolution S -> Cin over dY with the taps rotated and the channel axes swapped (k_split_pack mode 4),
//           Cin / 128 slices of 128 columns (64: one of 64); dW = k_split_wgrad on S x S tiles, rows = S, cols = Cin;
//   trunk   t_b = conv(y, W_b) + bias_b for all nb branches in one launch, written BRANCH-MAJOR [nb][B H W][S] (BC_BRANCH);
//           dy = sum_b rot(W_b) dT_b in one launch with one chain per element (BC_MULTI) from nb separate dT_b tensors;
//           dW [nb][S][S][3][3] = k_split_wgrad with rows = nb S, row tile b on dT_b and its own words (MULTI);
//   bias    db [nb][S] = the column sums of dT_b: pieces of HC_DB_PIECE rows per workgroup, each thread its rows in row order,
//           the threads of a column in order, the pieces in piece order (no atomics).
#define HC_SLICE_PIXELS 2048  // pixels per slice of the weight gradient: 108 slices at 470 x 470 (512 x 64: 127 MB of slabs)
#define HC_DB_PIECE 2048      // rows per piece of the bias gradient
#define HC_DB_THREADS 256

extern "C" int mssvt_head_conv_train_supported(int cin, int s, int nb) {
    return hc_cin(cin) && hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES ? 1 : 0;
}
// (cin, s) of the shared layer, or (s, s): the trunk
extern "C" int mssvt_head_conv_train_wgrad_slice_pixels(int cin, int s) { return (hc_cin(cin) || cin == s) && hc_s(s) ? HC_SLICE_PIXELS : 0; }
extern "C" int mssvt_head_conv_train_bias_piece_rows(int s) { return hc_s(s) ? HC_DB_PIECE : 0; }

static bool hc_bad_size(int B, int H, int W, int a, int b) { return B <= 0 || H <= 0 || W <= 0 || a <= 0 || b <= 0; }
// a host array of n device pointers: all present and 16-byte aligned
static bool hc_bad_ptrs(const float *const *p, int n) {
    if (!p) return true;
    for (int i = 0; i < n; ++i)
        if (!p[i] || bc_misaligned(p[i])) return true;
    return false;
}
static bc_ptrs hc_ptrs(const float *const *p, int n) {
    bc_ptrs out;
    for (int i = 0; i < BC_MAX_BRANCHES; ++i) out.p[i] = i < n ? p[i] : nullptr;
    return out;
}
static long long hc_slices(long long M) { return (M + HC_SLICE_PIXELS - 1) / HC_SLICE_PIXELS; }

// x (B, H, W, cin) -> y (B, H, W, s) = conv + shift (the blob of mssvt_head_conv_shared_pack with the BatchNorm pointers NULL);
// exp_workspace (B H W) int32 written here
extern "C" int mssvt_head_conv_shared_train(const float *x, int B, int H, int W, int cin, int s, const void *packed,
                                            int *exp_workspace, float *y, void *stream) {
    if (!x || !packed || !exp_workspace || !y || hc_bad_size(B, H, W, cin, s) || bc_misaligned(x) || bc_misaligned(y) ||
        bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    int status = hc_expmap(x, (long long)B * H * W, cin, exp_workspace, (hipStream_t)stream);
    if (status != MSSVT_OK) return status;
#define HC_GO(CI, S) \
    if (cin == CI && s == S) return hc_launch<CI, S, BC_ROWS>(x, CI, 0, B, H, W, packed, 1, exp_workspace, 1, 0, y, nullptr, stream);
    HC_GO(64, 32) HC_GO(64, 64) HC_GO(256, 32) HC_GO(256, 64) HC_GO(384, 32) HC_GO(384, 64) HC_GO(512, 32) HC_GO(512, 64)
#undef HC_GO
    return MSSVT_E_TOOLARGE;
}

// [words of dy: B H W int32, padded to 256 bytes][the blob of the convolution s -> cin: 64 bytes, scale, shift, 9 s cin weights]
extern "C" long long mssvt_head_conv_shared_dgrad_workspace_bytes(int B, int H, int W, int cin, int s) {
    if (hc_bad_size(B, H, W, cin, s) || !hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return 0;
    return bw_round256(4ll * B * H * W) + BC_HDR(1) + 8ll * cin + 36ll * cin * s;
}

// dy (B, H, W, s), weight (s, cin, 3, 3) as Conv2d holds it -> dx (B, H, W, cin)
extern "C" int mssvt_head_conv_shared_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int s, float *dx,
                                            void *workspace, void *stream) {
    if (!dy || !weight || !dx || !workspace || hc_bad_size(B, H, W, cin, s) || bc_misaligned(dy) || bc_misaligned(weight) ||
        bc_misaligned(dx) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    int *edy = reinterpret_cast<int *>(workspace);
    void *blob = edy + bw_round256(4 * M) / 4;
    const int ns = cin < 128 ? cin : 128;
    int status = bc_pack(weight, 4, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 3, s, cin, 0, ns, cin / ns, 0, 1, blob, st);
    if (status != MSSVT_OK) return status;
    status = hc_expmap(dy, M, s, edy, st);
    if (status != MSSVT_OK) return status;
#define HC_GO(S, NS)                                                                                                              \
    if (s == S && ns == NS)                                                                                                       \
        return bc_launch<S, NS, 3, false, BC_ROWS>(dy, S, 0, H, W, H, W, (int)M, blob, cin / NS, 3, 1, 1, edy, 1, 0, dx, nullptr, 0, \
                                                   0, st);
    HC_GO(32, 64) HC_GO(64, 64) HC_GO(32, 128) HC_GO(64, 128)
#undef HC_GO
    return MSSVT_E_TOOLARGE;
}

// [words of x: B H W int32, padded to 256 bytes][words of dy: the same][slices x 9 slabs of (s, cin) f32]
extern "C" long long mssvt_head_conv_shared_wgrad_workspace_bytes(int B, int H, int W, int cin, int s) {
    if (hc_bad_size(B, H, W, cin, s) || !hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return 0;
    const long long M = (long long)B * H * W;
    return 2 * bw_round256(4 * M) + hc_slices(M) * 9 * cin * s * 4;
}

// x (B, H, W, cin), dy (B, H, W, s) -> dw (s, cin, 3, 3)
extern "C" int mssvt_head_conv_shared_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int s, float *dw,
                                            void *workspace, void *stream) {
    if (!x || !dy || !dw || !workspace || hc_bad_size(B, H, W, cin, s) || bc_misaligned(x) || bc_misaligned(dy) ||
        bc_misaligned(dw) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    int *ex = reinterpret_cast<int *>(workspace), *edy = ex + bw_round256(4 * M) / 4;
    float *slab = reinterpret_cast<float *>(edy + bw_round256(4 * M) / 4);
    int status = hc_expmap(x, M, cin, ex, st);
    if (status != MSSVT_OK) return status;
    status = hc_expmap(dy, M, s, edy, st);
    if (status != MSSVT_OK) return status;
    // bw_launch(tapped, plain, .., cols, rows, ..): rows = s (dy, the plain operand), columns = cin (x, read at the tap's pixel)
    if (s == 32) return bw_launch<32, BW_TAPS3>(x, dy, H, W, (int)M, cin, s, 1, 9, HC_SLICE_PIXELS, ex, edy, slab, dw, st);
    return bw_launch<64, BW_TAPS3>(x, dy, H, W, (int)M, cin, s, 1, 9, HC_SLICE_PIXELS, ex, edy, slab, dw, st);
}

// ---- the bias gradient -----------------------------------------------------------------------------------------------------
// part [branch][piece][S]: thread (g, l) adds the float4 column l of rows g, g + G, .. of the piece in row order, then the G
// threads of a column are added in order of g
template <int S>
__global__ void __launch_bounds__(HC_DB_THREADS) k_hc_db_pieces(bc_ptrs dys, long long M, int pieces, float *part) {
    constexpr int LPR = S / 4, G = HC_DB_THREADS / LPR;
    __shared__ float4 sh[G][LPR];
    const int l = threadIdx.x % LPR, g = threadIdx.x / LPR, piece = blockIdx.x, br = blockIdx.y;
    const long long row0 = (long long)piece * HC_DB_PIECE;
    const int nrows = (int)min((long long)HC_DB_PIECE, M - row0);
    const float *base = dys.p[br] + row0 * S + 4 * l;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = g; r < nrows; r += G) {
        const float4 v = *reinterpret_cast<const float4 *>(base + (long long)r * S);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    sh[g][l] = a;
    __syncthreads();
    if (threadIdx.x < S) {
        const float *f = reinterpret_cast<const float *>(sh);
        float t = f[threadIdx.x];
        for (int j = 1; j < G; ++j) t += f[j * S + threadIdx.x];
        part[((size_t)br * pieces + piece) * S + threadIdx.x] = t;
    }
}

// db [branch][S]: the pieces in piece order; grid (nb), S threads
static __global__ void __launch_bounds__(64) k_hc_db_sum(const float *part, int pieces, int S, float *db) {
    const float *p = part + (size_t)blockIdx.x * pieces * S + threadIdx.x;
    float t = p[0];
    for (int i = 1; i < pieces; ++i) t += p[(size_t)i * S];
    db[blockIdx.x * S + threadIdx.x] = t;
}

// [nb x pieces x s f32]
extern "C" long long mssvt_head_conv_bgrad_workspace_bytes(int B, int H, int W, int s, int nb) {
    if (hc_bad_size(B, H, W, s, nb) || !hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return 0;
    return ((long long)B * H * W + HC_DB_PIECE - 1) / HC_DB_PIECE * nb * s * 4;
}

// host_dys: HOST array of nb device pointers, dT_b (B, H, W, s) each -> db [nb][s] (the shared layer: nb = 1)
extern "C" int mssvt_head_conv_bgrad(const float *const *host_dys, int B, int H, int W, int s, int nb, float *db, void *workspace,
                                     void *stream) {
    if (!db || !workspace || hc_bad_size(B, H, W, s, nb) || bc_misaligned(db) || bc_misaligned(workspace)) return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    if (hc_bad_ptrs(host_dys, nb)) return MSSVT_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    const int pieces = (int)((M + HC_DB_PIECE - 1) / HC_DB_PIECE);
    float *part = reinterpret_cast<float *>(workspace);
    if (s == 32) k_hc_db_pieces<32><<<dim3(pieces, nb), HC_DB_THREADS, 0, st>>>(hc_ptrs(host_dys, nb), M, pieces, part);
    else k_hc_db_pieces<64><<<dim3(pieces, nb), HC_DB_THREADS, 0, st>>>(hc_ptrs(host_dys, nb), M, pieces, part);
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    k_hc_db_sum<<<nb, s, 0, st>>>(part, pieces, s, db);
    return mssvt_launch_status();
}

// ---- the trunk ---------------------------------------------------------------------------------------------------------------
// y (B, H, W, s) -> t [nb][B H W][s] = conv_b + shift_b (the blob of mssvt_head_conv_trunk_pack with the BatchNorm pointers
// NULL); exp_workspace (B H W) int32 written here
extern "C" int mssvt_head_conv_trunk_train(const float *y, int B, int H, int W, int s, int nb, const void *packed,
                                           int *exp_workspace, float *t, void *stream) {
    if (!y || !packed || !exp_workspace || !t || hc_bad_size(B, H, W, s, nb) || bc_misaligned(y) || bc_misaligned(t) ||
        bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    int status = hc_expmap(y, (long long)B * H * W, s, exp_workspace, (hipStream_t)stream);
    if (status != MSSVT_OK) return status;
    if (s == 32) return hc_launch<32, 32, BC_BRANCH>(y, 32, 0, B, H, W, packed, nb, exp_workspace, 1, 0, t, nullptr, stream);
    return hc_launch<64, 64, BC_BRANCH>(y, 64, 0, B, H, W, packed, nb, exp_workspace, 1, 0, t, nullptr, stream);
}

// the power of two of ALL branches' weights (one accumulation chain reads them all) -> header record 0, scale 1, shift 0
static __global__ void __launch_bounds__(1024) k_hc_prep_multi(bc_ptrs w, int nb, int count, int ns, unsigned char *blob) {
    __shared__ int part[16];
    int m = 0;
    for (int b = 0; b < nb; ++b)
        for (int i = threadIdx.x; i < count; i += blockDim.x) m = max(m, bc_abs_bits(w.p[b][i]));
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (lane_id() == 0) part[threadIdx.x / MSSVT_WAVE] = m;
    __syncthreads();
    if (threadIdx.x < 16) {
        m = 0;
        for (int i = 0; i < 16; ++i) m = max(m, part[i]);
        int eb;
        const bool norm = pow2_norm_exponent(m, eb);
        const int word[2] = {norm ? 0x7F000000 - eb : 0x3F800000, norm ? eb : 0x3F800000};
        reinterpret_cast<int *>(blob)[threadIdx.x] = threadIdx.x < 2 ? word[threadIdx.x] : 0;
    }
    float *scale = reinterpret_cast<float *>(blob + BC_HDR(1));
    for (int c = threadIdx.x; c < ns; c += blockDim.x) {
        scale[c] = 1.f;
        scale[ns + c] = 0.f;
    }
}

// [words of the dT_b: nb B H W int32, padded to 256 bytes][the blob of the convolution nb s -> s]
extern "C" long long mssvt_head_conv_trunk_dgrad_workspace_bytes(int B, int H, int W, int s, int nb) {
    if (hc_bad_size(B, H, W, s, nb) || !hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return 0;
    return bw_round256(4ll * nb * B * H * W) + BC_HDR(1) + 8ll * s + 36ll * s * s * nb;
}

// host_dts / host_weights: HOST arrays of nb device pointers, dT_b (B, H, W, s) and W_b (s, s, 3, 3) -> dy (B, H, W, s)
extern "C" int mssvt_head_conv_trunk_dgrad(const float *const *host_dts, const float *const *host_weights, int B, int H, int W,
                                           int s, int nb, float *dy, void *workspace, void *stream) {
    if (!dy || !workspace || hc_bad_size(B, H, W, s, nb) || bc_misaligned(dy) || bc_misaligned(workspace)) return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    if (hc_bad_ptrs(host_dts, nb) || hc_bad_ptrs(host_weights, nb)) return MSSVT_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    int *edt = reinterpret_cast<int *>(workspace);
    unsigned char *blob = reinterpret_cast<unsigned char *>(edt + bw_round256(4 * nb * M) / 4);
    k_hc_prep_multi<<<1, 1024, 0, st>>>(hc_ptrs(host_weights, nb), nb, 9 * s * s, s, blob);
    int status = mssvt_launch_status();
    for (int b = 0; b < nb && status == MSSVT_OK; ++b) {
        k_split_pack<<<divup(9ll * s * s / 8, 256), 256, 0, st>>>(host_weights[b], 4, 3, s, s, s, 1, 0, 1, BC_HDR(1), blob, nb, b);
        status = mssvt_launch_status();
        if (status == MSSVT_OK) status = hc_expmap(host_dts[b], M, s, edt + (size_t)b * M, st);
    }
    if (status != MSSVT_OK) return status;
    if (s == 32)
        return bc_launch<32, 32, 3, false, BC_MULTI>(nullptr, 32, nb, H, W, H, W, (int)M, blob, 1, 3, 1, 1, edt, 1, 0, dy, nullptr, 0, 0,
                                                     st, hc_ptrs(host_dts, nb));
    return bc_launch<64, 64, 3, false, BC_MULTI>(nullptr, 64, nb, H, W, H, W, (int)M, blob, 1, 3, 1, 1, edt, 1, 0, dy, nullptr, 0, 0, st,
                                                 hc_ptrs(host_dts, nb));
}

// [words of y: B H W int32, padded to 256 bytes][words of the dT_b: nb B H W, padded][slices x 9 slabs of (nb s, s) f32]
extern "C" long long mssvt_head_conv_trunk_wgrad_workspace_bytes(int B, int H, int W, int s, int nb) {
    if (hc_bad_size(B, H, W, s, nb) || !hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return 0;
    const long long M = (long long)B * H * W;
    return bw_round256(4 * M) + bw_round256(4 * nb * M) + hc_slices(M) * 9 * nb * s * s * 4;
}

// y (B, H, W, s), host_dts: HOST array of nb device pointers dT_b (B, H, W, s) -> dw [nb][s][s][3][3]
extern "C" int mssvt_head_conv_trunk_wgrad(const float *y, const float *const *host_dts, int B, int H, int W, int s, int nb,
                                           float *dw, void *workspace, void *stream) {
    if (!y || !dw || !workspace || hc_bad_size(B, H, W, s, nb) || bc_misaligned(y) || bc_misaligned(dw) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    if (hc_bad_ptrs(host_dts, nb)) return MSSVT_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    int *ey = reinterpret_cast<int *>(workspace), *edt = ey + bw_round256(4 * M) / 4;
    float *slab = reinterpret_cast<float *>(edt + bw_round256(4 * nb * M) / 4);
    int status = hc_expmap(y, M, s, ey, st);
    for (int b = 0; b < nb && status == MSSVT_OK; ++b) status = hc_expmap(host_dts[b], M, s, edt + (size_t)b * M, st);
    if (status != MSSVT_OK) return status;
    // rows = nb s: row tile b is branch b (its own tensor and words), columns = s (y, read at the tap's pixel)
    if (s == 32)
        return bw_launch<32, BW_TAPS3, true>(y, nullptr, H, W, (int)M, s, nb * s, 1, 9, HC_SLICE_PIXELS, ey, edt, slab, dw, st, 0, 0,
                                             hc_ptrs(host_dts, nb));
    return bw_launch<64, BW_TAPS3, true>(y, nullptr, H, W, (int)M, s, nb * s, 1, 9, HC_SLICE_PIXELS, ey, edt, slab, dw, st, 0, 0,
                                         hc_ptrs(host_dts, nb));
}
