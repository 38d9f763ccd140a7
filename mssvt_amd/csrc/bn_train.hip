// bn_train.hip -- BatchNorm2d in TRAINING mode with an optional ReLU behind it, forward and backward, on dense channels-last
// fp32 tensors seen as a matrix of P = B H W rows by C channels, C in {32, 64, 128, 256}.  No matrix instructions, no float
// atomics, no host read: every sum has one fixed order, so the results are bit-identical from call to call.
//
// The rows are cut into PIECES of mssvt_bn_train_piece_rows(C) = 8192 / C rows (32 KiB of x; a function of C alone).  A
// workgroup of 256 threads owns a fixed run of consecutive pieces (bn_run: ceil(pieces / 1024) of them, so at most 1024
// workgroups).  Thread t holds the float4 column l = t % (C / 4) of the rows g, g + G, ..., g + 7 G of a piece, g = t / (C / 4),
// G = 1024 / C: eight 16-byte loads in flight per thread, one read of x per piece.
//
//   forward   k_bn_stats   per piece and channel, with the pivot K = the piece's first row: s1 = sum (x - K), s2 = sum (x - K)^2
//                          (eight terms per thread in row order, then the G threads of a channel in order through LDS);
//                          mean_i = K + s1 / n_i, M2_i = s2 - s1 (s1 / n_i), mean_i -> workspace, one lane per element;
//                          then the workgroup merges its own pieces in piece order: mean_b = K' + sum n_i (mean_i - K') / n_b
//                          with K' = its first mean_i, M2_b = sum M2_i + sum n_i (mean_i - mean_b)^2 -> workspace
//             k_bn_merge   per channel, the workgroups' (n_b, mean_b, M2_b) in order by the same two formulas (64 consecutive
//                          runs of partials, their sums added in run order): mean, M2 = sum M2_b + n_b (mean_b - mean)^2;
//                          save_mean, save_invstd = 1 / sqrt(M2 / P + eps) (IEEE division and square root), running buffers
//             k_bn_apply   y = (x - mean) invstd gamma + beta (bn_z, four roundings), ReLU, 16-byte loads and stores
//   backward  k_bn_bwd_reduce  per piece and channel: sum g and sum g xhat, g = dy [z > 0] with z RECOMPUTED from x by bn_z,
//                              added over the workgroup's pieces in piece order -> workspace
//             k_bn_bwd_merge   dbeta, dgamma over the workgroups in order as above; dbeta / P and dgamma / P to the workspace
//             k_bn_bwd_apply   dx = (gamma invstd) (g - dbeta / P - xhat dgamma / P)
//
// Every workspace word that is read was written by the launch before it.  tests/bn_train_ref.py derives the error bounds
// from exactly this arithmetic.
#include "common.hip.h"

#define BN_THREADS 256
#define BN_PIECE_FLOATS 8192  // a piece: 32 KiB of x
#define BN_ROWS 8             // rows of a piece per thread
#define BN_MAX_BLOCKS 1024    // workgroups of the two piece kernels
#define BN_RUNS 64            // runs of consecutive pieces in the merge kernels
#define BN_MERGE_THREADS (16 * BN_RUNS)
#define BN_MERGE_UNROLL 8
#define BN_MAX_ROWS 2147483647ll
#define BN_APPLY_UNROLL 4

static bool bn_channels(int C) { return C == 32 || C == 64 || C == 128 || C == 256; }
static bool bn_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static long long bn_pieces(long long P, int C) { return (P + BN_PIECE_FLOATS / C - 1) / (BN_PIECE_FLOATS / C); }
static int bn_run(long long pieces) { return (int)((pieces + BN_MAX_BLOCKS - 1) / BN_MAX_BLOCKS); }  // pieces per workgroup

extern "C" int mssvt_bn_train_supported(int C) { return bn_channels(C) ? 1 : 0; }
extern "C" int mssvt_bn_train_piece_rows(int C) { return bn_channels(C) ? BN_PIECE_FLOATS / C : 0; }
extern "C" int mssvt_bn_train_run_pieces(long long P, int C) {
    return (P < 2 || P > BN_MAX_ROWS || !bn_channels(C)) ? 0 : bn_run(bn_pieces(P, C));
}
// [pieces x C f32: the pieces' means][workgroups x C f32][workgroups x C f32][2 C f32]
extern "C" long long mssvt_bn_train_workspace_bytes(long long P, int C) {
    if (P < 2 || P > BN_MAX_ROWS || !bn_channels(C)) return 0;
    const long long pieces = bn_pieces(P, C), run = bn_run(pieces), blocks = (pieces + run - 1) / run;
    return ((pieces + 2 * blocks) * C + 2 * C) * 4;
}

// the pre-activation: ONE expression for the forward and for the backward's mask (-ffp-contract=off: four roundings)
__device__ __forceinline__ float bn_xhat(float x, float mean, float invstd) { return (x - mean) * invstd; }
__device__ __forceinline__ float bn_z(float x, float mean, float invstd, float g, float b) { return bn_xhat(x, mean, invstd) * g + b; }
__device__ __forceinline__ float bn_relu(float z) { return z <= 0.f ? 0.f : z; }  // keeps a NaN
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
// rows of part p when the P rows are cut every R rows: a piece, or a workgroup's run of pieces (the last may be short)
__device__ __forceinline__ float bn_piece_n(long long P, int R, int p) { return (float)(int)min((long long)R, P - (long long)p * R); }

template <int C>
__global__ __launch_bounds__(BN_THREADS) void k_bn_stats(const float *__restrict__ x, long long P, int pieces, int run,
                                                         float *pmean, float *__restrict__ bmean, float *__restrict__ bm2) {
    constexpr int LPR = C / 4, G = BN_THREADS / LPR, R = BN_PIECE_FLOATS / C;
    static_assert(R == BN_ROWS * G, "a thread holds BN_ROWS rows of a piece");
    __shared__ float4 sh1[G][LPR], sh2[G][LPR];
    const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
    const int first = blockIdx.x * run, last = min(first + run, pieces);
    float Kb = 0.f, S = 0.f, M = 0.f;  // (threads < C) the workgroup's pivot, sum n_i (mean_i - Kb) and sum M2_i, in piece order
    for (int piece = first; piece < last; ++piece) {
        const long long row0 = (long long)piece * R;
        const int nrows = (int)min((long long)R, P - row0);
        const float *base = x + row0 * C + 4 * l;
        const float4 K = ld4(base);
        float4 v[BN_ROWS];
#pragma unroll
        for (int k = 0; k < BN_ROWS; ++k) {
            const int row = k * G + g;
            v[k] = row < nrows ? ld4(base + (long long)row * C) : K;  // a row past the end: x - K = 0
        }
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
        for (int k = 0; k < BN_ROWS; ++k) {
            const float dx = v[k].x - K.x, dy = v[k].y - K.y, dz = v[k].z - K.z, dw = v[k].w - K.w;
            s1.x += dx; s1.y += dy; s1.z += dz; s1.w += dw;
            s2.x = fmaf(dx, dx, s2.x); s2.y = fmaf(dy, dy, s2.y); s2.z = fmaf(dz, dz, s2.z); s2.w = fmaf(dw, dw, s2.w);
        }
        sh1[g][l] = s1;
        sh2[g][l] = s2;
        __syncthreads();
        if (threadIdx.x < C) {
            const int c = threadIdx.x;
            const float *a = reinterpret_cast<const float *>(sh1), *b = reinterpret_cast<const float *>(sh2);
            float t1 = a[c], t2 = b[c];
#pragma unroll
            for (int j = 1; j < G; ++j) {
                t1 += a[j * C + c];
                t2 += b[j * C + c];
            }
            const float q = t1 / (float)nrows;
            const float m2 = t2 - t1 * q, mean_i = x[row0 * C + c] + q;
            pmean[(long long)piece * C + c] = mean_i;
            if (piece == first) Kb = mean_i;
            S += (float)nrows * (mean_i - Kb);
            M += m2 < 0.f ? 0.f : m2;  // (a NaN stays)
        }
        __syncthreads();
    }
    if (threadIdx.x < C) {  // the workgroup's own pieces -> one (mean, M2) per channel; it reads back what this thread wrote
        const int c = threadIdx.x;
        const float nb = (float)(int)min((long long)(last - first) * R, P - (long long)first * R);
        const float mean_b = Kb + S / nb;
        float Q = 0.f;
        for (int p = first; p < last; p += BN_MERGE_UNROLL) {
            float v[BN_MERGE_UNROLL];
#pragma unroll
            for (int u = 0; u < BN_MERGE_UNROLL; ++u) v[u] = p + u < last ? pmean[(long long)(p + u) * C + c] : mean_b;
#pragma unroll
            for (int u = 0; u < BN_MERGE_UNROLL; ++u)
                if (p + u < last) {
                    const float e = v[u] - mean_b;
                    Q += bn_piece_n(P, R, p + u) * (e * e);
                }
        }
        bmean[(long long)blockIdx.x * C + c] = mean_b;
        bm2[(long long)blockIdx.x * C + c] = M + Q;
    }
}

// the partials [p0, p1) of run `run` (BN_RUNS consecutive runs cover all of them; a run may be empty)
__device__ __forceinline__ void bn_run_range(int pieces, int run, int *p0, int *p1) {
    const int len = (pieces + BN_RUNS - 1) / BN_RUNS;
    *p0 = min(run * len, pieces);
    *p1 = min(*p0 + len, pieces);
}
__device__ __forceinline__ float bn_sum_runs(const float (*sh)[16], int ch) {
    float s = sh[0][ch];
#pragma unroll 8
    for (int j = 1; j < BN_RUNS; ++j) s += sh[j][ch];
    return s;
}

// The workgroups' partials (`pieces` of them, of R rows each, the last may be short) in order.  Grid C / 16, BN_MERGE_THREADS
// threads; thread (run, channel) = (t / 16, t % 16).  The loads of BN_MERGE_UNROLL partials are issued together (the loop is
// bound by their latency), the sums stay in order.
__global__ __launch_bounds__(BN_MERGE_THREADS) void k_bn_merge(const float *__restrict__ pmean, const float *__restrict__ pm2,
                                                               long long P, int C, int R, int pieces, float eps, float momentum,
                                                               float *__restrict__ running_mean, float *__restrict__ running_var,
                                                               float *__restrict__ save_mean, float *__restrict__ save_invstd) {
    __shared__ float sh[BN_RUNS][16];
    const int ch = threadIdx.x & 15, run = threadIdx.x >> 4, c = blockIdx.x * 16 + ch;
    int p0, p1;
    bn_run_range(pieces, run, &p0, &p1);
    const float K = pmean[c], Pf = (float)P;
    float s = 0.f;
    for (int p = p0; p < p1; p += BN_MERGE_UNROLL) {
        float v[BN_MERGE_UNROLL];
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u) v[u] = p + u < p1 ? pmean[(long long)(p + u) * C + c] : K;
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u)
            if (p + u < p1) s += bn_piece_n(P, R, p + u) * (v[u] - K);
    }
    sh[run][ch] = s;
    __syncthreads();
    const float mean = K + bn_sum_runs(sh, ch) / Pf;
    __syncthreads();
    float q = 0.f;
    for (int p = p0; p < p1; p += BN_MERGE_UNROLL) {
        float v[BN_MERGE_UNROLL], w[BN_MERGE_UNROLL];
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u) {
            v[u] = p + u < p1 ? pmean[(long long)(p + u) * C + c] : mean;
            w[u] = p + u < p1 ? pm2[(long long)(p + u) * C + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u)
            if (p + u < p1) {
                const float e = v[u] - mean;
                q += w[u] + bn_piece_n(P, R, p + u) * (e * e);
            }
    }
    sh[run][ch] = q;
    __syncthreads();
    if (run == 0) {
        const float var = bn_sum_runs(sh, ch) / Pf;
        save_mean[c] = mean;
        save_invstd[c] = 1.0f / sqrtf(var + eps);
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (var * (Pf / (Pf - 1.0f)));
    }
}

template <int C>
__global__ __launch_bounds__(BN_THREADS) void k_bn_apply(const float *__restrict__ x, long long n4, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, int relu, float *__restrict__ y) {
    constexpr int LPR = C / 4;  // LPR divides BN_THREADS: a thread stays on its four channels
    const int l = threadIdx.x % LPR;
    const float4 m = ld4(mean + 4 * l), s = ld4(invstd + 4 * l), g = ld4(gamma + 4 * l), b = ld4(beta + 4 * l);
    const long long i0 = (long long)blockIdx.x * (BN_THREADS * BN_APPLY_UNROLL) + threadIdx.x;
    float4 v[BN_APPLY_UNROLL];
#pragma unroll
    for (int k = 0; k < BN_APPLY_UNROLL; ++k) {
        const long long i = i0 + k * BN_THREADS;
        v[k] = i < n4 ? ld4(x + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < BN_APPLY_UNROLL; ++k) {
        const long long i = i0 + k * BN_THREADS;
        float4 z = make_float4(bn_z(v[k].x, m.x, s.x, g.x, b.x), bn_z(v[k].y, m.y, s.y, g.y, b.y),
                               bn_z(v[k].z, m.z, s.z, g.z, b.z), bn_z(v[k].w, m.w, s.w, g.w, b.w));
        if (relu) z = make_float4(bn_relu(z.x), bn_relu(z.y), bn_relu(z.z), bn_relu(z.w));
        if (i < n4) *reinterpret_cast<float4 *>(y + 4 * i) = z;
    }
}

// g = dy [z > 0] (relu) or dy; *gx = g xhat
__device__ __forceinline__ float bn_g(float x, float dy, float mean, float invstd, float gamma, float beta, int relu, float *xhat) {
    *xhat = bn_xhat(x, mean, invstd);
    return (!relu || bn_z(x, mean, invstd, gamma, beta) > 0.f) ? dy : 0.f;
}

template <int C>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_reduce(const float *__restrict__ x, const float *__restrict__ dy, long long P,
                                                              int pieces, int run, const float *__restrict__ mean,
                                                              const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, int relu, float *__restrict__ pb,
                                                              float *__restrict__ pg) {
    constexpr int LPR = C / 4, G = BN_THREADS / LPR, R = BN_PIECE_FLOATS / C;
    __shared__ float4 sh1[G][LPR], sh2[G][LPR];
    const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
    const float4 m = ld4(mean + 4 * l), s = ld4(invstd + 4 * l), ga = ld4(gamma + 4 * l), be = ld4(beta + 4 * l);
    const int first = blockIdx.x * run, last = min(first + run, pieces);
    float sb = 0.f, sg = 0.f;  // (threads < C) the workgroup's sums over its pieces, in piece order
    for (int piece = first; piece < last; ++piece) {
        const long long row0 = (long long)piece * R;
        const int nrows = (int)min((long long)R, P - row0);
        const long long off = row0 * C + 4 * l;
        float4 v[BN_ROWS], w[BN_ROWS];
#pragma unroll
        for (int k = 0; k < BN_ROWS; ++k) {
            const int row = k * G + g;
            const bool live = row < nrows;
            v[k] = ld4(x + off + (live ? (long long)row * C : 0));  // a row past the end: the piece's first row with dy = 0
            w[k] = live ? ld4(dy + off + (long long)row * C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
        for (int k = 0; k < BN_ROWS; ++k) {
            float h;
            float t = bn_g(v[k].x, w[k].x, m.x, s.x, ga.x, be.x, relu, &h); s1.x += t; s2.x += t * h;
            t = bn_g(v[k].y, w[k].y, m.y, s.y, ga.y, be.y, relu, &h); s1.y += t; s2.y += t * h;
            t = bn_g(v[k].z, w[k].z, m.z, s.z, ga.z, be.z, relu, &h); s1.z += t; s2.z += t * h;
            t = bn_g(v[k].w, w[k].w, m.w, s.w, ga.w, be.w, relu, &h); s1.w += t; s2.w += t * h;
        }
        sh1[g][l] = s1;
        sh2[g][l] = s2;
        __syncthreads();
        if (threadIdx.x < C) {
            const int c = threadIdx.x;
            const float *a = reinterpret_cast<const float *>(sh1), *b = reinterpret_cast<const float *>(sh2);
            float t1 = a[c], t2 = b[c];
#pragma unroll
            for (int j = 1; j < G; ++j) {
                t1 += a[j * C + c];
                t2 += b[j * C + c];
            }
            sb += t1;
            sg += t2;
        }
        __syncthreads();
    }
    if (threadIdx.x < C) {
        pb[(long long)blockIdx.x * C + threadIdx.x] = sb;
        pg[(long long)blockIdx.x * C + threadIdx.x] = sg;
    }
}

__global__ __launch_bounds__(BN_MERGE_THREADS) void k_bn_bwd_merge(const float *__restrict__ pb, const float *__restrict__ pg,
                                                                   long long P, int C, int pieces, float *__restrict__ dgamma,
                                                                   float *__restrict__ dbeta, float *__restrict__ scaled) {
    __shared__ float shb[BN_RUNS][16], shg[BN_RUNS][16];
    const int ch = threadIdx.x & 15, run = threadIdx.x >> 4, c = blockIdx.x * 16 + ch;
    int p0, p1;
    bn_run_range(pieces, run, &p0, &p1);
    float sb = 0.f, sg = 0.f;
    for (int p = p0; p < p1; p += BN_MERGE_UNROLL) {
        float v[BN_MERGE_UNROLL], w[BN_MERGE_UNROLL];
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u) {
            v[u] = p + u < p1 ? pb[(long long)(p + u) * C + c] : 0.f;
            w[u] = p + u < p1 ? pg[(long long)(p + u) * C + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < BN_MERGE_UNROLL; ++u)
            if (p + u < p1) {
                sb += v[u];
                sg += w[u];
            }
    }
    shb[run][ch] = sb;
    shg[run][ch] = sg;
    __syncthreads();
    if (run == 0) {
        const float db = bn_sum_runs(shb, ch), dg = bn_sum_runs(shg, ch), Pf = (float)P;
        dbeta[c] = db;
        dgamma[c] = dg;
        scaled[c] = db / Pf;
        scaled[C + c] = dg / Pf;
    }
}

template <int C>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_apply(const float *__restrict__ x, const float *__restrict__ dy, long long n4,
                                                             const float *__restrict__ mean, const float *__restrict__ invstd,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             const float *__restrict__ scaled, int relu, float *__restrict__ dx) {
    constexpr int LPR = C / 4;
    const int l = threadIdx.x % LPR;
    const float4 m = ld4(mean + 4 * l), s = ld4(invstd + 4 * l), ga = ld4(gamma + 4 * l), be = ld4(beta + 4 * l);
    const float4 a = ld4(scaled + 4 * l), b = ld4(scaled + C + 4 * l);
    const float4 f = make_float4(ga.x * s.x, ga.y * s.y, ga.z * s.z, ga.w * s.w);
    const long long i0 = (long long)blockIdx.x * (BN_THREADS * BN_APPLY_UNROLL) + threadIdx.x;
    float4 v[BN_APPLY_UNROLL], w[BN_APPLY_UNROLL];
#pragma unroll
    for (int k = 0; k < BN_APPLY_UNROLL; ++k) {
        const long long i = i0 + k * BN_THREADS;
        v[k] = i < n4 ? ld4(x + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        w[k] = i < n4 ? ld4(dy + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < BN_APPLY_UNROLL; ++k) {
        const long long i = i0 + k * BN_THREADS;
        float4 o;
        float h;
        float t = bn_g(v[k].x, w[k].x, m.x, s.x, ga.x, be.x, relu, &h); o.x = f.x * (t - a.x - h * b.x);
        t = bn_g(v[k].y, w[k].y, m.y, s.y, ga.y, be.y, relu, &h); o.y = f.y * (t - a.y - h * b.y);
        t = bn_g(v[k].z, w[k].z, m.z, s.z, ga.z, be.z, relu, &h); o.z = f.z * (t - a.z - h * b.z);
        t = bn_g(v[k].w, w[k].w, m.w, s.w, ga.w, be.w, relu, &h); o.w = f.w * (t - a.w - h * b.w);
        if (i < n4) *reinterpret_cast<float4 *>(dx + 4 * i) = o;
    }
}

static int bn_check(long long P, int C, const void *const *ptrs, int nptrs) {
    for (int i = 0; i < nptrs; ++i)
        if (!ptrs[i] || bn_misaligned(ptrs[i])) return MSSVT_E_BADARG;
    if (P < 2 || C <= 0) return MSSVT_E_BADARG;
    if (!bn_channels(C) || P > BN_MAX_ROWS) return MSSVT_E_TOOLARGE;
    return MSSVT_OK;
}

#define BN_DISPATCH(KERNEL, GRID, ...)                                                                      \
    switch (C) {                                                                                            \
    case 32: hipLaunchKernelGGL(KERNEL<32>, dim3(GRID), dim3(BN_THREADS), 0, st, __VA_ARGS__); break;       \
    case 64: hipLaunchKernelGGL(KERNEL<64>, dim3(GRID), dim3(BN_THREADS), 0, st, __VA_ARGS__); break;       \
    case 128: hipLaunchKernelGGL(KERNEL<128>, dim3(GRID), dim3(BN_THREADS), 0, st, __VA_ARGS__); break;     \
    default: hipLaunchKernelGGL(KERNEL<256>, dim3(GRID), dim3(BN_THREADS), 0, st, __VA_ARGS__); break;      \
    }

extern "C" int mssvt_bn_train_fwd(const float *x, long long P, int C, const float *gamma, const float *beta, float eps,
                                  float momentum, float *running_mean, float *running_var, int relu, float *y, float *save_mean,
                                  float *save_invstd, void *workspace, void *stream) {
    const void *ptrs[] = {x, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, workspace};
    const int bad = bn_check(P, C, ptrs, 9);
    if (bad != MSSVT_OK) return bad;
    hipStream_t st = (hipStream_t)stream;
    const int pieces = (int)bn_pieces(P, C), run = bn_run(pieces), blocks = (pieces + run - 1) / run;
    float *pmean = reinterpret_cast<float *>(workspace), *bmean = pmean + (long long)pieces * C, *bm2 = bmean + (long long)blocks * C;
    BN_DISPATCH(k_bn_stats, blocks, x, P, pieces, run, pmean, bmean, bm2)
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    hipLaunchKernelGGL(k_bn_merge, dim3(C / 16), dim3(BN_MERGE_THREADS), 0, st, bmean, bm2, P, C, run * (BN_PIECE_FLOATS / C), blocks, eps,
                       momentum, running_mean, running_var, save_mean, save_invstd);
    status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    const long long n4 = P * (C / 4);
    const int grid = divup(n4, BN_THREADS * BN_APPLY_UNROLL);
    BN_DISPATCH(k_bn_apply, grid, x, n4, save_mean, save_invstd, gamma, beta, relu, y)
    return mssvt_launch_status();
}

extern "C" int mssvt_bn_train_bwd(const float *x, const float *dy, long long P, int C, const float *gamma, const float *beta,
                                  const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                                  float *dbeta, void *workspace, void *stream) {
    const void *ptrs[] = {x, dy, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta, workspace};
    const int bad = bn_check(P, C, ptrs, 10);
    if (bad != MSSVT_OK) return bad;
    hipStream_t st = (hipStream_t)stream;
    const int pieces = (int)bn_pieces(P, C), run = bn_run(pieces), blocks = (pieces + run - 1) / run;
    float *pb = reinterpret_cast<float *>(workspace), *pg = pb + (long long)blocks * C, *scaled = pg + (long long)blocks * C;
    BN_DISPATCH(k_bn_bwd_reduce, blocks, x, dy, P, pieces, run, save_mean, save_invstd, gamma, beta, relu, pb, pg)
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    hipLaunchKernelGGL(k_bn_bwd_merge, dim3(C / 16), dim3(BN_MERGE_THREADS), 0, st, pb, pg, P, C, blocks, dgamma, dbeta, scaled);
    status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    const long long n4 = P * (C / 4);
    const int grid = divup(n4, BN_THREADS * BN_APPLY_UNROLL);
    BN_DISPATCH(k_bn_bwd_apply, grid, x, dy, n4, save_mean, save_invstd, gamma, beta, scaled, relu, dx)
    return mssvt_launch_status();
}
