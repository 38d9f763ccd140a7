// bev_conv.hip -- the dense 3x3 / 1x1 convolutions behind the sparse backbone in eval mode on NHWC fp32 tensors (ref: the
// Conv2d + BatchNorm2d + ReLU triples of pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-39 and
// pcdet/models/backbones_2d/base_bev_backbone.py:30-78), on the split-fp16 v_mfma_f32_16x16x32_f16 kernel of
// split_conv.hip.h, which holds the arithmetic, the pipeline and the blob layout.  What is this file's own:
//   * the entry points mssvt_bev_conv_supported / _pack_bytes / _pack and mssvt_bev_conv (k_split_expmap over the input, then
//     k_split_conv with run-time taps: 3x3 at stride 1 / 2 and dilation 1 / 2 with padding = dilation, or 1x1);
//   * the channel shapes of bc_channels; Cout = 256 is two slices of 128 columns;
//   * one header record for the whole tensor: ONE power of two for all weights, k and kbase unused (zero);
//   * mssvt_bev_conv_into, the same layers writing a channel slice of a wider tensor (BC_ROWS_INTO), and mssvt_bev_up2_*, the
//     2 x 2 stride-2 transposed deblock (ref base_bev_backbone.py:52-63) as a 1 x 1 layer of 4 Cout columns (BC_UP2): the blob
//     is the BEV blob of that layer, column ph Cout + n with ph = dy 2 + dx, scale / shift repeated per phase;
//   * mssvt_bev_conv_wgrad_*, the weight gradient of the 3 x 3 stride-1 layers with cin = cout for the training path
//     (split_wgrad.hip.h: a GEMM over pixels in slices, partial slabs in a workspace, added in slice order);
//   * mssvt_bev_deblock_*, the backward of the transposed deblocks whose kernel equals their stride s in {1, 2}: the weight
//     gradient is the same GEMM with the phases (dy, dx) as taps (BW_PHASES), the input gradient is k_split_conv over dY with
//     the weight tensor (cin, cout, s, s) packed as the Conv2d weight (out, in, ky, kx) it already is: s x s taps at stride s;
//   * mssvt_bev_down_*, the backward of the 3 x 3 stride-2 layer (zero padding 1): the weight gradient is the same GEMM over
//     the OUTPUT pixels with X read at (2 oy + ky - 1, 2 ox + kx - 1) (BW_DOWN), the input gradient is k_split_conv over dY as
//     the four parity phases of dX in one launch (BC_DOWN2: 4 + 2 + 2 + 1 taps, the 9 taps of the weight each used once).
#include "split_conv.hip.h"
#include "split_wgrad.hip.h"

#define BC_NS(COUT) ((COUT) < 128 ? (COUT) : 128)  // output channels per workgroup (slice)

static bool bc_channels(int cin, int cout) {
    return (cin == 128 && cout == 128) || (cin == 128 && cout == 256) || (cin == 256 && cout == 256) ||
           (cin == 32 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 64);
}

extern "C" int mssvt_bev_conv_supported(int ksize, int cin, int cout, int stride, int dilation) {
    if (!bc_channels(cin, cout)) return 0;
    if (ksize == 3) return (stride == 1 || stride == 2) && (dilation == 1 || dilation == 2) ? 1 : 0;
    return ksize == 1 && stride == 1 && dilation == 1 ? 1 : 0;
}

extern "C" long long mssvt_bev_conv_pack_bytes(int ksize, int cin, int cout) {
    if (!mssvt_bev_conv_supported(ksize, cin, cout, 1, 1)) return 0;
    return BC_HDR(cout / BC_NS(cout)) + 8ll * cout + 4ll * ksize * ksize * cin * cout;
}

extern "C" int mssvt_bev_conv_pack(const float *weight, int transposed, const float *bias, const float *bn_weight,
                                   const float *bn_bias, const float *bn_mean, const float *bn_var, float bn_eps, int ksize,
                                   int cin, int cout, void *packed, void *stream) {
    if (!weight || !packed || ksize <= 0 || cin <= 0 || cout <= 0 || (transposed && ksize != 1) ||
        bc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!mssvt_bev_conv_supported(ksize, cin, cout, 1, 1)) return MSSVT_E_TOOLARGE;
    return bc_pack(weight, transposed, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, ksize, cin, cout, 0, BC_NS(cout),
                   cout / BC_NS(cout), 0, 1, packed, (hipStream_t)stream);
}

// x (B, H, W, cin) f32, packed = mssvt_bev_conv_pack's blob, exp_workspace (B H W) int32 (written here, no need to clear),
// y (B, Ho, Wo, cout) f32 with Ho = (H + 2 p - 2 d (k - 1) / 2 - 1) / stride + 1, p = d for 3 x 3 and 0 for 1 x 1; INTO: y's pixels
// are rows of ystride floats of which the layer writes channels [ybase, ybase + cout)
template <bool INTO>
static int bc_conv(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout, int stride, int dilation,
                   int relu, int *exp_workspace, float *y, int ystride, int ybase, hipStream_t st) {
    if (!x || !packed || !exp_workspace || !y || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || ksize <= 0 ||
        stride <= 0 || dilation <= 0 || bc_misaligned(x) || bc_misaligned(y) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (INTO && (ystride <= 0 || ybase < 0 || ystride % 4 || ybase % 4 || (long long)ybase + cout > ystride)) return MSSVT_E_BADARG;
    if (!mssvt_bev_conv_supported(ksize, cin, cout, stride, dilation) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;  // padding = dilation (3 x 3) / 0 (1 x 1)
#define BC_GO(CI, NSL)                                                                                                      \
    if (cin == CI && BC_NS(cout) == NSL) {                                                                                  \
        const int status = bc_expmap<CI, CI / 4>(x, (long long)B * H * W, exp_workspace, st);                               \
        if (status != MSSVT_OK) return status;                                                                              \
        return bc_launch<CI, NSL, 0, false, INTO ? BC_ROWS_INTO : BC_ROWS>(x, CI, 0, H, W, Ho, Wo, B * Ho * Wo, packed,      \
                                                                           cout / NSL, ksize, stride, dilation, exp_workspace, \
                                                                           1, relu, y, nullptr, ystride, ybase, st);         \
    }
    BC_GO(128, 128) BC_GO(256, 128) BC_GO(32, 32) BC_GO(32, 64) BC_GO(64, 64)
#undef BC_GO
    return MSSVT_E_TOOLARGE;
}

extern "C" int mssvt_bev_conv(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout, int stride,
                              int dilation, int relu, int *exp_workspace, float *y, void *stream) {
    return bc_conv<false>(x, B, H, W, cin, packed, ksize, cout, stride, dilation, relu, exp_workspace, y, 0, 0, (hipStream_t)stream);
}

extern "C" int mssvt_bev_conv_into(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout,
                                   int stride, int dilation, int relu, int *exp_workspace, float *y, int ystride, int ybase,
                                   void *stream) {
    return bc_conv<true>(x, B, H, W, cin, packed, ksize, cout, stride, dilation, relu, exp_workspace, y, ystride, ybase,
                         (hipStream_t)stream);
}

// ---- up-2: ConvTranspose2d(cin, cout, 2, stride = 2) + BatchNorm2d + ReLU as the 1 x 1 layer of 4 cout columns (BC_UP2) -----
extern "C" int mssvt_bev_up2_supported(int cin, int cout) { return (cin == 256 && cout == 256) || (cin == 64 && cout == 32) ? 1 : 0; }

extern "C" long long mssvt_bev_up2_pack_bytes(int cin, int cout) {
    if (!mssvt_bev_up2_supported(cin, cout)) return 0;
    return BC_HDR(1) + 8ll * 4 * cout + 4ll * cin * 4 * cout;
}

extern "C" int mssvt_bev_up2_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                  const float *bn_mean, const float *bn_var, float bn_eps, int cin, int cout, void *packed,
                                  void *stream) {
    if (!weight || !packed || cin <= 0 || cout <= 0 || bc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!mssvt_bev_up2_supported(cin, cout)) return MSSVT_E_TOOLARGE;
    return bc_pack(weight, 2, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, 1, cin, 4 * cout, 0, BC_NS(cout),
                   4 * cout / BC_NS(cout), 0, 1, packed, (hipStream_t)stream);
}

// x (B, H, W, cin) f32, packed = mssvt_bev_up2_pack's blob, exp_workspace (B H W) int32 (written here), y (B, 2 H, 2 W, ystride)
// f32 of which channels [ybase, ybase + cout) are written
extern "C" int mssvt_bev_up2(const float *x, int B, int H, int W, int cin, const void *packed, int cout, int relu,
                             int *exp_workspace, float *y, int ystride, int ybase, void *stream) {
    if (!x || !packed || !exp_workspace || !y || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || ystride <= 0 || ybase < 0 ||
        ystride % 4 || ybase % 4 || (long long)ybase + cout > ystride || bc_misaligned(x) || bc_misaligned(y) || bc_misaligned(packed))
        return MSSVT_E_BADARG;
    // the OUTPUT pixels, 4 B H W, are what the kernel's addresses count
    if (!mssvt_bev_up2_supported(cin, cout) || (long long)B * H * W > (0x7FFFFFFFll - 4 * BC_BLOCK_PIXELS) / 4) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
#define BC_GO(CI, CO)                                                                                                         \
    if (cin == CI && cout == CO) {                                                                                            \
        const int status = bc_expmap<CI, CI / 4>(x, (long long)B * H * W, exp_workspace, st);                                 \
        if (status != MSSVT_OK) return status;                                                                                \
        return bc_launch<CI, BC_NS(CO), 0, false, BC_UP2>(x, CI, 0, H, W, H, W, B * H * W, packed, 4 * CO / BC_NS(CO), 1, 1, 1, \
                                                          exp_workspace, 1, relu, y, nullptr, ystride, ybase, st);            \
    }
    BC_GO(256, 256) BC_GO(64, 32)
#undef BC_GO
    return MSSVT_E_TOOLARGE;
}

// ---- the weight gradient of the 3 x 3 stride-1 layers with cin = cout (the kernels: split_wgrad.hip.h) ----------------------
extern "C" int mssvt_bev_conv_wgrad_supported(int ksize, int cin, int cout, int stride, int dilation) {
    return ksize == 3 && stride == 1 && (dilation == 1 || dilation == 2) && bw_channels(cin, cout) ? 1 : 0;
}

extern "C" int mssvt_bev_conv_wgrad_slice_pixels(int cin, int cout) { return bw_channels(cin, cout) ? bw_slice_pixels(cin) : 0; }

// [words of x: B H W int32, padded to 256 bytes][words of dy: the same][slices x 9 slabs of (cout, cin) f32]
extern "C" long long mssvt_bev_conv_wgrad_workspace_bytes(int B, int H, int W, int ksize, int cin, int cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !mssvt_bev_conv_wgrad_supported(ksize, cin, cout, 1, 1) || bc_too_many_pixels(B, H, W)) return 0;
    const long long M = (long long)B * H * W, nslices = (M + bw_slice_pixels(cin) - 1) / bw_slice_pixels(cin);
    return 2 * bw_round256(4 * M) + nslices * 9 * cin * cout * 4;
}

extern "C" int mssvt_bev_conv_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, int ksize, int dilation,
                                    float *dw, void *workspace, void *stream) {
    if (!x || !dy || !dw || !workspace || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || ksize <= 0 || dilation <= 0 ||
        bc_misaligned(x) || bc_misaligned(dy) || bc_misaligned(dw) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!mssvt_bev_conv_wgrad_supported(ksize, cin, cout, 1, dilation) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W;
    int *ex = reinterpret_cast<int *>(workspace), *edy = ex + bw_round256(4 * M) / 4;
    float *slab = reinterpret_cast<float *>(edy + bw_round256(4 * M) / 4);
#define BW_GO(CH, TILE)                                                                                           \
    if (cin == CH) {                                                                                              \
        int status = bc_expmap<CH, CH / 4>(x, M, ex, st);                                                         \
        if (status != MSSVT_OK) return status;                                                                    \
        status = bc_expmap<CH, CH / 4>(dy, M, edy, st);                                                           \
        if (status != MSSVT_OK) return status;                                                                    \
        return bw_launch<TILE, BW_TAPS3>(x, dy, H, W, (int)M, cin, cout, dilation, 9, bw_slice_pixels(cin), ex, edy, \
                                         slab, dw, st);                                                           \
    }
    BW_GO(128, 128) BW_GO(256, 128) BW_GO(32, 32) BW_GO(64, 64)
#undef BW_GO
    return MSSVT_E_TOOLARGE;
}

// ---- the backward of ConvTranspose2d(cin, cout, s, stride = s), s in {1, 2}: x / dx (B, H, W, cin), dy (B, s H, s W, cout) -------
extern "C" int mssvt_bev_deblock_train_supported(int stride, int cin, int cout) { return bw_deblock_shape(stride, cin, cout) ? 1 : 0; }

extern "C" int mssvt_bev_deblock_wgrad_slice_pixels(int stride, int cin, int cout) {
    return bw_deblock_shape(stride, cin, cout) ? bw_deblock_slice_pixels(cin) : 0;
}

// the kernels' addresses count the s s B H W pixels of dy
static bool bd_too_many_pixels(int B, int H, int W, int stride) {
    return (long long)B * H * W > (0x7FFFFFFFll - 4 * BC_BLOCK_PIXELS) / (stride * stride);
}

// [words of x: B H W int32, padded to 256 bytes][words of dy: s s B H W, padded][slices x s s slabs of (cin, cout) f32]
extern "C" long long mssvt_bev_deblock_wgrad_workspace_bytes(int B, int H, int W, int stride, int cin, int cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !bw_deblock_shape(stride, cin, cout) || bd_too_many_pixels(B, H, W, stride)) return 0;
    const long long M = (long long)B * H * W, slice = bw_deblock_slice_pixels(cin), nslices = (M + slice - 1) / slice;
    return bw_round256(4 * M) + bw_round256(4 * stride * stride * M) + nslices * stride * stride * cin * cout * 4;
}

extern "C" int mssvt_bev_deblock_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, int stride, float *dw,
                                       void *workspace, void *stream) {
    if (!x || !dy || !dw || !workspace || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || stride <= 0 || bc_misaligned(x) ||
        bc_misaligned(dy) || bc_misaligned(dw) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!bw_deblock_shape(stride, cin, cout) || bd_too_many_pixels(B, H, W, stride)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)B * H * W, Mdy = M * stride * stride;
    int *ex = reinterpret_cast<int *>(workspace), *edy = ex + bw_round256(4 * M) / 4;
    float *slab = reinterpret_cast<float *>(edy + bw_round256(4 * Mdy) / 4);
    // bw_launch(tapped, plain, .., cols, rows, ..): rows = cin (x, the plain operand), columns = cout (dy, read at the phase's pixel)
#define BD_GO(CI, CO, TILE)                                                                                                   \
    if (cin == CI && cout == CO) {                                                                                            \
        int status = bc_expmap<CI, CI / 4>(x, M, ex, st);                                                                     \
        if (status != MSSVT_OK) return status;                                                                                \
        status = bc_expmap<CO, CO / 4>(dy, Mdy, edy, st);                                                                     \
        if (status != MSSVT_OK) return status;                                                                                \
        return bw_launch<TILE, BW_PHASES>(dy, x, H, W, (int)M, cout, cin, stride, stride * stride,                            \
                                          bw_deblock_slice_pixels(cin), edy, ex, slab, dw, st);                       \
    }
    BD_GO(128, 256, 128) BD_GO(256, 256, 128) BD_GO(32, 64, 32) BD_GO(64, 32, 32)
#undef BD_GO
    return MSSVT_E_TOOLARGE;
}

// the blob of the Conv2d layer cout -> cin with s x s taps (one header record: 64 bytes, scale, shift, the weight blocks)
static long long bd_blob_bytes(int stride, int cin, int cout) { return BC_HDR(1) + 8ll * cin + 4ll * stride * stride * cin * cout; }

// [words of dy: s s B H W int32, padded to 256 bytes][the blob]
extern "C" long long mssvt_bev_deblock_dgrad_workspace_bytes(int B, int H, int W, int stride, int cin, int cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !bw_deblock_shape(stride, cin, cout) || bd_too_many_pixels(B, H, W, stride)) return 0;
    return bw_round256(4ll * stride * stride * B * H * W) + bd_blob_bytes(stride, cin, cout);
}

extern "C" int mssvt_bev_deblock_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int cout, int stride,
                                       float *dx, void *workspace, void *stream) {
    if (!dy || !weight || !dx || !workspace || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || stride <= 0 ||
        bc_misaligned(dy) || bc_misaligned(weight) || bc_misaligned(dx) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!bw_deblock_shape(stride, cin, cout) || bd_too_many_pixels(B, H, W, stride)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long Mdy = (long long)B * H * W * stride * stride;
    int *edy = reinterpret_cast<int *>(workspace);
    void *blob = edy + bw_round256(4 * Mdy) / 4;
    // a Conv2d of CO input and CI output channels over dy (B, s H, s W): s x s taps, stride s, no padding, output H x W
#define BD_GO(CI, CO)                                                                                                         \
    if (cin == CI && cout == CO) {                                                                                            \
        int status = bc_pack(weight, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, stride, CO, CI, 0, BC_NS(CI),       \
                             CI / BC_NS(CI), 0, 1, blob, st);                                                                 \
        if (status != MSSVT_OK) return status;                                                                                \
        status = bc_expmap<CO, CO / 4>(dy, Mdy, edy, st);                                                                     \
        if (status != MSSVT_OK) return status;                                                                                \
        return bc_launch<CO, BC_NS(CI), 0, false, BC_ROWS>(dy, CO, 0, stride * H, stride * W, H, W, B * H * W, blob,          \
                                                           CI / BC_NS(CI), stride, stride, 1, edy, 1, 0, dx, nullptr, 0, 0, st); \
    }
    BD_GO(128, 256) BD_GO(256, 256) BD_GO(32, 64) BD_GO(64, 32)
#undef BD_GO
    return MSSVT_E_TOOLARGE;
}

// ---- the backward of Conv2d(cin, cout, 3, stride = 2, padding = 1): x / dx (B, H, W, cin), dy (B, Ho, Wo, cout) -------------------
extern "C" int mssvt_bev_down_train_supported(int cin, int cout) { return bw_down_shape(cin, cout) ? 1 : 0; }

extern "C" int mssvt_bev_down_wgrad_slice_pixels(int cin, int cout) { return bw_down_shape(cin, cout) ? bw_down_slice_pixels(cin) : 0; }

// [words of x: B H W int32, padded to 256 bytes][words of dy: B Ho Wo, padded][slices x 9 slabs of (cout, cin) f32]
extern "C" long long mssvt_bev_down_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !bw_down_shape(cin, cout) || bc_too_many_pixels(B, H, W)) return 0;
    const long long M = (long long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1), slice = bw_down_slice_pixels(cin);
    return bw_round256(4ll * B * H * W) + bw_round256(4 * M) + (M + slice - 1) / slice * 9 * cin * cout * 4;
}

extern "C" int mssvt_bev_down_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, float *dw,
                                    void *workspace, void *stream) {
    if (!x || !dy || !dw || !workspace || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || bc_misaligned(x) ||
        bc_misaligned(dy) || bc_misaligned(dw) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!bw_down_shape(cin, cout) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long Mx = (long long)B * H * W, M = (long long)B * Ho * Wo;
    int *ex = reinterpret_cast<int *>(workspace), *edy = ex + bw_round256(4 * Mx) / 4;
    float *slab = reinterpret_cast<float *>(edy + bw_round256(4 * M) / 4);
    // bw_launch(tapped, plain, .., cols, rows, ..): rows = cout (dy, the plain operand), columns = cin (x, read at the tap's pixel)
#define BD_GO(CI, CO, TILE)                                                                                                  \
    if (cin == CI && cout == CO) {                                                                                           \
        int status = bc_expmap<CI, CI / 4>(x, Mx, ex, st);                                                                   \
        if (status != MSSVT_OK) return status;                                                                               \
        status = bc_expmap<CO, CO / 4>(dy, M, edy, st);                                                                      \
        if (status != MSSVT_OK) return status;                                                                               \
        return bw_launch<TILE, BW_DOWN>(x, dy, Ho, Wo, (int)M, cin, cout, 2, 9, bw_down_slice_pixels(cin), ex, edy, slab, dw, \
                                        st, H, W);                                                                           \
    }
    BD_GO(128, 256, 128) BD_GO(32, 64, 32)
#undef BD_GO
    return MSSVT_E_TOOLARGE;
}

// the blob of the four phase convolutions cout -> cin, 9 taps in all (one header record: 64 bytes, scale, shift, the blocks)
static long long bdn_blob_bytes(int cin, int cout) { return BC_HDR(1) + 8ll * cin + 4ll * 9 * cin * cout; }

// [words of dy: B Ho Wo int32, padded to 256 bytes][the blob]
extern "C" long long mssvt_bev_down_dgrad_workspace_bytes(int B, int H, int W, int cin, int cout) {
    if (B <= 0 || H <= 0 || W <= 0 || !bw_down_shape(cin, cout) || bc_too_many_pixels(B, H, W)) return 0;
    return bw_round256(4ll * B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1)) + bdn_blob_bytes(cin, cout);
}

extern "C" int mssvt_bev_down_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int cout, float *dx,
                                    void *workspace, void *stream) {
    if (!dy || !weight || !dx || !workspace || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || bc_misaligned(dy) ||
        bc_misaligned(weight) || bc_misaligned(dx) || bc_misaligned(workspace))
        return MSSVT_E_BADARG;
    if (!bw_down_shape(cin, cout) || bc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long M = (long long)B * Ho * Wo;
    int *edy = reinterpret_cast<int *>(workspace);
    void *blob = edy + bw_round256(4 * M) / 4;
    // four convolutions of CO input and CI output channels over dy (B, Ho, Wo), one per parity of dx's pixel: BC_DOWN2
#define BD_GO(CI, CO)                                                                                                       \
    if (cin == CI && cout == CO) {                                                                                          \
        int status = bc_pack(weight, 3, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 3, CO, CI, 0, BC_NS(CI),          \
                             CI / BC_NS(CI), 0, 1, blob, st);                                                               \
        if (status != MSSVT_OK) return status;                                                                              \
        status = bc_expmap<CO, CO / 4>(dy, M, edy, st);                                                                     \
        if (status != MSSVT_OK) return status;                                                                              \
        return bc_launch<CO, BC_NS(CI), 0, false, BC_DOWN2>(dy, CO, 0, Ho, Wo, H, W, (int)M, blob, CI / BC_NS(CI), 3, 2, 1, \
                                                            edy, 1, 0, dx, nullptr, 0, 0, st);                              \
    }
    BD_GO(128, 256) BD_GO(32, 64)
#undef BD_GO
    return MSSVT_E_TOOLARGE;
}
