// The multi-interest encoder of MIND and ComirecDR (rec_pangu/models/layers/multi_interest.py:56-161, CapsuleNetwork) and the
// hard readout of rec_pangu/models/sequence/mind.py:44-49 / comirec.py:100-105, gfx950.
//
// (a) ComirecDR's position-batched projection  U[b, s, n] = sum_d W[s, n, d] X[b, s, d]  (n < N = K D): ONE launch for all L
//     positions, grid (batch tile, N tile, position), on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32: an fp32 FMA
//     chain, so no tolerance argument is needed).  The reference's [B, L, K D, D] product is never formed and U stays
//     [B, L, K D]: the routing launch takes strides.  Backward: dX[b, s, :] = dU[b, s, :] W[s] (contraction over N) and
//     dW[s] = sum_b dU[b, s, :]^T X[b, s, :] — one workgroup per (position, 32 output rows, batch split) walks its rows front to
//     back; above 512 rows the batch is split (32 splits at the most) and a second launch adds the partial sums in split
//     order, so the contraction order is fixed and no float atomics exist.
// (b) Routing: three rounds per (b, k) exactly as multi_interest.py:125-154, one wave per (b, k), the K waves of a sample in
//     one workgroup, the sample's U tile(s) in LDS with a one-float row pad (lane = column for c^T U, lane = position for
//     U v: both walks conflict-free), reductions by fixed-order butterflies.  The backward recomputes the rounds, keeps
//     p_i, s_i, v_i in registers (3 L + 6 D floats per (b, k)) and writes dU as the rank-5 sum
//         dU = sum_{i<=2} c_i ds_i^T + sum_{i<=1} ddelta_i v_i^T
//     with no accumulation buffer; with interest stride 0 (MIND: all K interests read one [L, D] tile) the K contributions
//     are added in interest order inside the workgroup.
// (c) Readout: k*[b] = argmax_k out[b, k, :] . E[target[b], :] (first maximum wins), best[b] = out[b, k*[b]]; the backward
//     scatters dbest to the chosen interest and writes exact zeros elsewhere.
#include "common.h"

#include <math.h>

namespace {

constexpr int CAP_TB = 64;    // projection forward: batch rows per workgroup (two 32-row tiles per wave)
constexpr int CAP_TN = 128;   // projection forward: output columns per workgroup (a wave per 32)
constexpr int CAP_TBX = 32;   // projection dX: batch rows per workgroup
constexpr int CAP_NK = 64;    // projection dX / dW: contraction chunk staged in LDS
constexpr int CAP_WROWS = 512;       // projection dW: batch rows per split (at least), CAP_WSPLITS splits at the most
constexpr int CAP_WSPLITS = 32;
constexpr int CAP_MAX_D = 128;
constexpr int CAP_MAX_N = 2048;
constexpr int CAP_MAX_K = 8;
constexpr int CAP_MAX_L = 64;
constexpr int CAP_LDS = 144 * 1024;  // routing: bytes of LDS the sample's tiles may take
constexpr float CAP_EPS = 1e-9f;

// ---- (a) projection ------------------------------------------------------------------------------------------------------
// grid (ceil(B / 64), ceil(N / 128), L), 256 threads; dynamic LDS: xs [64][Dp + 4], ws [128][Dp + 4], Dp = D rounded up to 8
__global__ __launch_bounds__(256) void cap_project_fwd_kernel(const float *__restrict__ X, const float *__restrict__ W,
                                                              int64_t B, int64_t L, int N, int D, int Dp,
                                                              float *__restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float cap_lds[];
    const int ld = Dp + 4;
    float *xs = cap_lds, *ws = xs + CAP_TB * ld;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5, j = 32 * w + i;
    const int64_t b0 = (int64_t)blockIdx.x * CAP_TB, s = blockIdx.z;
    const int n0 = blockIdx.y * CAP_TN;
    for (int idx = tid; idx < CAP_TB * Dp; idx += 256) {
        const int row = idx / Dp, k = idx % Dp;
        const int64_t b = b0 + row;
        xs[row * ld + k] = (b < B && k < D) ? X[(b * L + s) * D + k] : 0.f;
    }
    for (int idx = tid; idx < CAP_TN * Dp; idx += 256) {
        const int row = idx / Dp, k = idx % Dp, n = n0 + row;
        ws[row * ld + k] = (n < N && k < D) ? W[(s * N + n) * D + k] : 0.f;
    }
    __syncthreads();
    if (n0 + 32 * w >= N) return;  // (uniform over the wave, behind the only barrier)
    f32x16 acc0 = {0}, acc1 = {0};
    for (int kq = 0; kq < Dp / 8; ++kq) {
        const int k = kq * 8 + 4 * h;
        const f32x4 w4 = *reinterpret_cast<const f32x4 *>(&ws[j * ld + k]);
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(&xs[i * ld + k]);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(&xs[(32 + i) * ld + k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], w4[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], w4[e], acc1, 0, 0, 0);
        }
    }
    const int n = n0 + j;
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t ba = b0 + rp_mfma32_row(r, h), bb = ba + 32;
        if (ba < B) U[(ba * L + s) * N + n] = acc0[r];
        if (bb < B) U[(bb * L + s) * N + n] = acc1[r];
    }
}

// dX[b, s, d] = sum_n dU[b, s, n] W[s, n, d]: grid (ceil(B / 32), L), 256 threads, wave w owns the columns [32 w, 32 w + 32)
__global__ __launch_bounds__(256) void cap_project_bwd_x_kernel(const float *__restrict__ dU, const float *__restrict__ W,
                                                                int64_t B, int64_t L, int N, int D, int Dp32,
                                                                float *__restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float as[CAP_TBX * (CAP_NK + 4)];
    __shared__ float ws[CAP_NK * CAP_MAX_D];
    constexpr int lda = CAP_NK + 4;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5, j = 32 * w + i;
    const int64_t b0 = (int64_t)blockIdx.x * CAP_TBX, s = blockIdx.y;
    const bool mine = 32 * w < Dp32;
    f32x16 acc = {0};
    for (int nc = 0; nc < N; nc += CAP_NK) {
        for (int idx = tid; idx < CAP_TBX * CAP_NK; idx += 256) {
            const int row = idx / CAP_NK, k = idx % CAP_NK;
            const int64_t b = b0 + row;
            as[row * lda + k] = (b < B && nc + k < N) ? dU[(b * L + s) * N + nc + k] : 0.f;
        }
        for (int idx = tid; idx < CAP_NK * Dp32; idx += 256) {
            const int k = idx / Dp32, d = idx % Dp32;
            ws[k * Dp32 + d] = (nc + k < N && d < D) ? W[(s * N + nc + k) * D + d] : 0.f;
        }
        __syncthreads();
        if (mine) {
            for (int kq = 0; kq < CAP_NK / 8; ++kq) {
                const int k = kq * 8 + 4 * h;
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&as[i * lda + k]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], ws[(k + e) * Dp32 + j], acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!mine || j >= D) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t b = b0 + rp_mfma32_row(r, h);
        if (b < B) dX[(b * L + s) * D + j] = acc[r];
    }
}

// dW[s, n, d] = sum_b dU[b, s, n] X[b, s, d]: grid (ceil(N / 32), L, splits), 256 threads; the workgroup walks ITS `rows` batch
// rows front to back in chunks of 64, wave w owns the columns d in [32 w, 32 w + 32) of the 32 output rows.  One split writes
// dW itself; several write their partial sums to part [splits][L][N][D], which cap_project_bwd_w_finish_kernel adds in split order
__global__ __launch_bounds__(256) void cap_project_bwd_w_kernel(const float *__restrict__ dU, const float *__restrict__ X,
                                                                int64_t B, int64_t L, int N, int D, int Dp32, int64_t rows,
                                                                float *__restrict__ part, float *__restrict__ dW) {
    __shared__ float ds[CAP_NK * 32];
    __shared__ float xs[CAP_NK * CAP_MAX_D];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5, j = 32 * w + i;
    const int n0 = blockIdx.x * 32;
    const int64_t s = blockIdx.y, lo = (int64_t)blockIdx.z * rows, hi = lo + rows < B ? lo + rows : B;
    const bool mine = 32 * w < Dp32;
    f32x16 acc = {0};
    for (int64_t bc = lo; bc < hi; bc += CAP_NK) {
        for (int idx = tid; idx < CAP_NK * 32; idx += 256) {
            const int k = idx / 32, n = n0 + idx % 32;
            const int64_t b = bc + k;
            ds[idx] = (b < hi && n < N) ? dU[(b * L + s) * N + n] : 0.f;
        }
        for (int idx = tid; idx < CAP_NK * Dp32; idx += 256) {
            const int k = idx / Dp32, d = idx % Dp32;
            const int64_t b = bc + k;
            xs[k * Dp32 + d] = (b < hi && d < D) ? X[(b * L + s) * D + d] : 0.f;
        }
        __syncthreads();
        if (mine) {
            for (int k = h; k < CAP_NK; k += 2)  // (one product takes two batch rows: lane half h supplies row k)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[k * 32 + i], xs[k * Dp32 + j], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (!mine || j >= D) return;
    float *dst = part != nullptr ? part + (int64_t)blockIdx.z * L * N * D : dW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = n0 + rp_mfma32_row(r, h);
        if (n < N) dst[(s * N + n) * D + j] = acc[r];
    }
}

__global__ __launch_bounds__(256) void cap_project_bwd_w_finish_kernel(const float *__restrict__ part, int splits, int64_t total,
                                                                       float *__restrict__ dW) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = 0.f;
    for (int q = 0; q < splits; ++q) s += part[q * total + e];
    dW[e] = s;
}

// ---- (b) routing ---------------------------------------------------------------------------------------------------------
struct CapRounds {
    float p[3], c[3], s0[3], s1[3], v0[3], v1[3], n[3];
};

// the three rounds of one (b, k) on one wave; u: the [L][ld] tile in LDS; bl: this lane's initial logit (lane = position)
__device__ __forceinline__ void cap_rounds(const float *u, int ld, int L, int D, int lane, float bl, bool m, CapRounds &R) {
    const bool u0 = lane < D, u1 = lane + 64 < D, pos = lane < L;
    const int lrow = pos ? lane : L - 1;
    const int dlo = D < 64 ? D : 64;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float mx = rp_lane_max(pos ? bl : -INFINITY);
        const float e = pos ? expf(bl - mx) : 0.f;
        const float p = e / rp_lane_sum(e);
        const float c = m ? p : 0.f;
        float a0 = 0.f, a1 = 0.f;
        for (int l = 0; l < L; ++l) {
            const float cl = __shfl(c, l);
            if (u0) a0 += cl * u[l * ld + lane];
            if (u1) a1 += cl * u[l * ld + lane + 64];
        }
        const float n = rp_lane_sum(a0 * a0 + a1 * a1);
        const float f = n / (1.f + n) / sqrtf(n + CAP_EPS);
        R.p[i] = p, R.c[i] = c, R.s0[i] = a0, R.s1[i] = a1, R.n[i] = n;
        R.v0[i] = f * a0, R.v1[i] = f * a1;
        if (i < 2) {
            float delta = 0.f;
            for (int d = 0; d < dlo; ++d) delta += u[lrow * ld + d] * __shfl(R.v0[i], d);
            for (int d = 64; d < D; ++d) delta += u[lrow * ld + d] * __shfl(R.v1[i], d - 64);
            bl += delta;
        }
    }
}

// tiles of the sample -> LDS: ntile x [L][D + 1] from U[b sb + kt sk + l sl + d]
__device__ __forceinline__ void cap_stage(const float *__restrict__ U, int64_t base, int64_t sk, int64_t sl, int ntile, int L,
                                          int D, float *lds) {
    const int ld = D + 1, per = L * D;
    for (int idx = threadIdx.x; idx < ntile * per; idx += blockDim.x) {
        const int kt = idx / per, rem = idx % per, l = rem / D, d = rem % D;
        lds[(kt * L + l) * ld + d] = U[base + kt * sk + l * sl + d];
    }
}

// grid B, block 64 K; dynamic LDS: (sk == 0 ? 1 : K) tiles
__global__ __launch_bounds__(512) void cap_route_fwd_kernel(const float *__restrict__ U, int64_t sb, int64_t sk, int64_t sl,
                                                            const float *__restrict__ mask, const float *__restrict__ b0,
                                                            int K, int L, int D, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float cap_lds[];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63, ld = D + 1;
    const int64_t b = blockIdx.x;
    cap_stage(U, b * sb, sk, sl, sk == 0 ? 1 : K, L, D, cap_lds);
    __syncthreads();
    const float *u = cap_lds + (sk == 0 ? 0 : k * L * ld);
    const bool pos = lane < L;
    const bool m = pos && mask[b * L + lane] != 0.f;
    const float bl = (pos && b0 != nullptr) ? b0[(b * K + k) * L + lane] : 0.f;
    CapRounds R;
    cap_rounds(u, ld, L, D, lane, bl, m, R);
    float *o = out + (b * K + k) * D;
    if (lane < D) o[lane] = R.v0[2];
    if (lane + 64 < D) o[lane + 64] = R.v1[2];
}

// grid B, block 64 K; dynamic LDS: sk == 0 ? 2 tiles (U, and the sum of the K contributions) : K tiles
__global__ __launch_bounds__(512) void cap_route_bwd_kernel(const float *__restrict__ U, int64_t sb, int64_t sk, int64_t sl,
                                                            const float *__restrict__ mask, const float *__restrict__ b0,
                                                            const float *__restrict__ dout, int K, int L, int D, int stop_grad,
                                                            float *__restrict__ dU) {
    extern __shared__ __attribute__((aligned(16))) float cap_lds[];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63, ld = D + 1;
    const int64_t b = blockIdx.x;
    cap_stage(U, b * sb, sk, sl, sk == 0 ? 1 : K, L, D, cap_lds);
    __syncthreads();
    const float *u = cap_lds + (sk == 0 ? 0 : k * L * ld);
    const bool pos = lane < L, u0 = lane < D, u1 = lane + 64 < D;
    const int lrow = pos ? lane : L - 1;
    const int dlo = D < 64 ? D : 64;
    const bool m = pos && mask[b * L + lane] != 0.f;
    const float bl = (pos && b0 != nullptr) ? b0[(b * K + k) * L + lane] : 0.f;
    CapRounds R;
    cap_rounds(u, ld, L, D, lane, bl, m, R);

    float ds0[3] = {0.f, 0.f, 0.f}, ds1[3] = {0.f, 0.f, 0.f}, dd[2] = {0.f, 0.f};
    float g0 = u0 ? dout[(b * K + k) * D + lane] : 0.f, g1 = u1 ? dout[(b * K + k) * D + lane + 64] : 0.f;
    float db = 0.f;  // gradient of the logits the round ABOVE reads (lane = position)
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        if (stop_grad && i < 2) break;  // rounds 0 and 1 read a detached U: nothing reaches it through them
        if (i < 2) {                    // b_{i+1} = b_i + U v_i: ddelta_i = db, dv_i = sum_l ddelta_i[l] U[l, :]
            dd[i] = db;
            g0 = 0.f, g1 = 0.f;
            for (int l = 0; l < L; ++l) {
                const float t = __shfl(db, l);
                if (u0) g0 += t * u[l * ld + lane];
                if (u1) g1 += t * u[l * ld + lane + 64];
            }
        }
        // squash: v = f(n) s, n = |s|^2  ->  ds = f g + 2 f'(n) (g . s) s
        const float n = R.n[i], rs = sqrtf(n + CAP_EPS), f = n / (1.f + n) / rs;
        const float fp = 1.f / ((1.f + n) * (1.f + n) * rs) - n / (2.f * (1.f + n) * (n + CAP_EPS) * rs);
        const float gs = rp_lane_sum(g0 * R.s0[i] + g1 * R.s1[i]);
        ds0[i] = f * g0 + 2.f * fp * gs * R.s0[i];
        ds1[i] = f * g1 + 2.f * fp * gs * R.s1[i];
        if (i > 0) {  // dc[l] = U[l, :] . ds, then through the masked softmax into the logits of this round
            float dc = 0.f;
            for (int d = 0; d < dlo; ++d) dc += u[lrow * ld + d] * __shfl(ds0[i], d);
            for (int d = 64; d < D; ++d) dc += u[lrow * ld + d] * __shfl(ds1[i], d - 64);
            dc = m ? dc : 0.f;
            const float tot = rp_lane_sum(R.p[i] * dc);
            db += R.p[i] * (dc - tot);
        }
    }
    // dU[l, :] = sum_i c_i[l] ds_i + sum_{i<=1} ddelta_i[l] v_i
    float *acc = cap_lds + L * ld;  // (shared form only: the second tile)
    for (int kk = 0; kk < (sk == 0 ? K : 1); ++kk) {
        if (sk != 0 || kk == k) {
            for (int l = 0; l < L; ++l) {
                const float c0 = __shfl(R.c[0], l), c1 = __shfl(R.c[1], l), c2 = __shfl(R.c[2], l);
                const float e0 = __shfl(dd[0], l), e1 = __shfl(dd[1], l);
                const float x0 = (((c0 * ds0[0] + c1 * ds0[1]) + c2 * ds0[2]) + e0 * R.v0[0]) + e1 * R.v0[1];
                const float x1 = (((c0 * ds1[0] + c1 * ds1[1]) + c2 * ds1[2]) + e0 * R.v1[0]) + e1 * R.v1[1];
                if (sk != 0) {
                    float *o = dU + b * sb + k * sk + l * sl;
                    if (u0) o[lane] = x0;
                    if (u1) o[lane + 64] = x1;
                } else {
                    if (u0) acc[l * ld + lane] = kk == 0 ? x0 : acc[l * ld + lane] + x0;
                    if (u1) acc[l * ld + lane + 64] = kk == 0 ? x1 : acc[l * ld + lane + 64] + x1;
                }
            }
        }
        if (sk == 0) __syncthreads();  // (sk is a kernel argument: every wave takes the same branch)
    }
    if (sk == 0) {
        for (int idx = threadIdx.x; idx < L * D; idx += blockDim.x) {
            const int l = idx / D, d = idx % D;
            dU[b * sb + l * sl + d] = acc[l * ld + d];
        }
    }
}

// ---- (c) readout ---------------------------------------------------------------------------------------------------------
// one wave per batch row, four per workgroup
__global__ __launch_bounds__(256) void cap_pick_fwd_kernel(const float *__restrict__ I, const float *__restrict__ E, int64_t V,
                                                           const int64_t *__restrict__ target, int64_t B, int K, int D,
                                                           float *__restrict__ best, int32_t *__restrict__ kidx,
                                                           int32_t *__restrict__ err_flag) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int64_t t = target[b];
    if (t < 0 || t >= V) {
        if (lane == 0) *err_flag = 1;
        t = 0;
    }
    const float *e = E + t * D, *rows = I + b * K * D;
    float top = 0.f;
    int kb = 0;
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += rows[k * D + d] * e[d];
        s = rp_lane_sum(s);
        if (k == 0 || s > top) top = s, kb = k;  // (strict: the first maximum wins)
    }
    for (int d = lane; d < D; d += 64) best[b * D + d] = rows[kb * D + d];
    if (lane == 0) kidx[b] = kb;
}

__global__ __launch_bounds__(256) void cap_pick_bwd_kernel(const float *__restrict__ dbest, const int32_t *__restrict__ kidx,
                                                           int64_t total, int K, int D, float *__restrict__ dout) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx % D);
    const int64_t bk = idx / D, b = bk / K;
    dout[idx] = (int)(bk % K) == kidx[b] ? dbest[b * D + d] : 0.f;
}

#define CAP_CHECK_PROJECT(what)                                                                                          \
    RP_REQUIRE(B >= 0 && B <= (int64_t)INT32_MAX && L >= 1 && L <= 65535 && D >= 1 && D <= CAP_MAX_D && N >= 1 &&         \
                   N <= CAP_MAX_N,                                                                                       \
               what ": need 0 <= B < 2^31, 1 <= L <= 65535, 1 <= D <= %d and 1 <= K D <= %d (got B=%lld L=%lld KD=%d D=%d)", \
               CAP_MAX_D, CAP_MAX_N, (long long)B, (long long)L, N, D)

// dW: splits of the batch and rows per split (a multiple of the staged chunk, so every split but the last is full)
int cap_w_splits(int64_t B, int64_t *rows) {
    int64_t n = rp_cdiv(B, CAP_WROWS);
    n = n < 1 ? 1 : (n > CAP_WSPLITS ? CAP_WSPLITS : n);
    *rows = rp_cdiv(rp_cdiv(B, n), CAP_NK) * CAP_NK;
    return (int)rp_cdiv(B > 0 ? B : 1, *rows > 0 ? *rows : 1);
}

bool cap_route_fits(int K, int L, int D) {
    return K >= 1 && K <= CAP_MAX_K && L >= 1 && L <= CAP_MAX_L && D >= 1 && D <= CAP_MAX_D &&
           sizeof(float) * (size_t)(K > 2 ? K : 2) * L * (D + 1) <= (size_t)CAP_LDS;
}

#define CAP_CHECK_ROUTE(what)                                                                                              \
    RP_REQUIRE(B >= 0 && B <= (int64_t)INT32_MAX && cap_route_fits(K, L, D),                                               \
               what ": need 0 <= B < 2^31, 1 <= K <= %d, 1 <= L <= %d, 1 <= D <= %d and 4 max(K, 2) L (D + 1) <= %d bytes " \
                    "(got B=%lld K=%d L=%d D=%d)",                                                                        \
               CAP_MAX_K, CAP_MAX_L, CAP_MAX_D, CAP_LDS, (long long)B, K, L, D);                                           \
    RP_REQUIRE(sb >= 1 && sl >= D && (sk == 0 || sk >= D), what ": strides must be sb >= 1, sl >= D and sk == 0 or sk >= D")

}  // namespace

extern "C" int rp_capsule_geometry(int *proj_tb, int *proj_tn, int *max_k, int *max_l, int *max_d, int *lds_bytes) {
    RP_REQUIRE(proj_tb && proj_tn && max_k && max_l && max_d && lds_bytes, "capsule_geometry: null pointer");
    *proj_tb = CAP_TB, *proj_tn = CAP_TN, *max_k = CAP_MAX_K, *max_l = CAP_MAX_L, *max_d = CAP_MAX_D, *lds_bytes = CAP_LDS;
    return RP_OK;
}

extern "C" int rp_capsule_project_fwd(const float *X, const float *W, int64_t B, int64_t L, int N, int D, float *U,
                                      rp_stream_t stream) {
    CAP_CHECK_PROJECT("capsule_project_fwd");
    RP_REQUIRE(X && W && U, "capsule_project_fwd: null pointer");
    if (B == 0) return RP_OK;
    const int Dp = rp_round_up(D, 8);
    const size_t lds = sizeof(float) * (size_t)(CAP_TB + CAP_TN) * (Dp + 4);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cap_project_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(cap_project_fwd_kernel, dim3((unsigned)rp_cdiv(B, CAP_TB), (unsigned)rp_cdiv(N, CAP_TN), (unsigned)L),
                       dim3(256), (unsigned)lds, (hipStream_t)stream, X, W, B, L, N, D, Dp, U);
    RP_LAUNCH_CHECK("capsule_project_fwd");
    return RP_OK;
}

extern "C" int rp_capsule_project_bwd_x(const float *dU, const float *W, int64_t B, int64_t L, int N, int D, float *dX,
                                        rp_stream_t stream) {
    CAP_CHECK_PROJECT("capsule_project_bwd_x");
    RP_REQUIRE(dU && W && dX, "capsule_project_bwd_x: null pointer");
    if (B == 0) return RP_OK;
    hipLaunchKernelGGL(cap_project_bwd_x_kernel, dim3((unsigned)rp_cdiv(B, CAP_TBX), (unsigned)L), dim3(256), 0,
                       (hipStream_t)stream, dU, W, B, L, N, D, rp_round_up(D, 32), dX);
    RP_LAUNCH_CHECK("capsule_project_bwd_x");
    return RP_OK;
}

extern "C" int rp_capsule_workspace_bytes(int64_t B, int64_t L, int N, int D, size_t *bytes) {
    RP_REQUIRE(bytes, "capsule_workspace_bytes: null pointer");
    CAP_CHECK_PROJECT("capsule_workspace_bytes");
    int64_t rows;
    const int splits = cap_w_splits(B, &rows);
    *bytes = splits > 1 ? sizeof(float) * (size_t)splits * (size_t)L * N * D : 0;
    return RP_OK;
}

extern "C" int rp_capsule_project_bwd_w(const float *dU, const float *X, int64_t B, int64_t L, int N, int D, float *dW,
                                        void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    CAP_CHECK_PROJECT("capsule_project_bwd_w");
    RP_REQUIRE(dU && X && dW, "capsule_project_bwd_w: null pointer");
    int64_t rows;
    const int splits = cap_w_splits(B, &rows);
    const int64_t total = L * N * D;
    RP_REQUIRE(splits == 1 || (workspace && workspace_bytes >= sizeof(float) * (size_t)splits * (size_t)total),
               "capsule_project_bwd_w: workspace missing or too small");
    float *part = splits > 1 ? static_cast<float *>(workspace) : nullptr;
    // (B == 0 still launches: dW is WRITTEN, zeros then)
    hipLaunchKernelGGL(cap_project_bwd_w_kernel, dim3((unsigned)rp_cdiv(N, 32), (unsigned)L, (unsigned)splits), dim3(256), 0,
                       (hipStream_t)stream, dU, X, B, L, N, D, rp_round_up(D, 32), rows, part, dW);
    RP_LAUNCH_CHECK("capsule_project_bwd_w");
    if (splits > 1) {
        hipLaunchKernelGGL(cap_project_bwd_w_finish_kernel, dim3((unsigned)rp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float *)part, splits, total, dW);
        RP_LAUNCH_CHECK("capsule_project_bwd_w (splits)");
    }
    return RP_OK;
}

extern "C" int rp_capsule_route_fwd(const float *U, int64_t sb, int64_t sk, int64_t sl, const float *mask, const float *b0,
                                    int64_t B, int K, int L, int D, float *out, rp_stream_t stream) {
    CAP_CHECK_ROUTE("capsule_route_fwd");
    RP_REQUIRE(U && mask && out, "capsule_route_fwd: null pointer");
    if (B == 0) return RP_OK;
    const size_t lds = sizeof(float) * (size_t)(sk == 0 ? 1 : K) * L * (D + 1);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cap_route_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(cap_route_fwd_kernel, dim3((unsigned)B), dim3(64 * K), (unsigned)lds, (hipStream_t)stream, U, sb, sk, sl,
                       mask, b0, K, L, D, out);
    RP_LAUNCH_CHECK("capsule_route_fwd");
    return RP_OK;
}

extern "C" int rp_capsule_route_bwd(const float *U, int64_t sb, int64_t sk, int64_t sl, const float *mask, const float *b0,
                                    const float *dout, int64_t B, int K, int L, int D, int stop_grad, float *dU,
                                    rp_stream_t stream) {
    CAP_CHECK_ROUTE("capsule_route_bwd");
    RP_REQUIRE(U && mask && dout && dU, "capsule_route_bwd: null pointer");
    if (B == 0) return RP_OK;
    const size_t lds = sizeof(float) * (size_t)(sk == 0 ? 2 : K) * L * (D + 1);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cap_route_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(cap_route_bwd_kernel, dim3((unsigned)B), dim3(64 * K), (unsigned)lds, (hipStream_t)stream, U, sb, sk, sl,
                       mask, b0, dout, K, L, D, stop_grad, dU);
    RP_LAUNCH_CHECK("capsule_route_bwd");
    return RP_OK;
}

extern "C" int rp_interest_pick_fwd(const float *interests, const float *E, int64_t V, const int64_t *target, int64_t B, int K,
                                    int D, float *best, int32_t *kidx, int32_t *err_flag, rp_stream_t stream) {
    RP_REQUIRE(interests && E && target && best && kidx && err_flag, "interest_pick_fwd: null pointer");
    RP_REQUIRE(B >= 0 && B <= (int64_t)INT32_MAX && K >= 1 && D >= 1 && V >= 1, "interest_pick_fwd: need 0 <= B < 2^31 and K, D, V >= 1");
    if (B == 0) return RP_OK;
    hipLaunchKernelGGL(cap_pick_fwd_kernel, dim3((unsigned)rp_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, interests, E, V,
                       target, B, K, D, best, kidx, err_flag);
    RP_LAUNCH_CHECK("interest_pick_fwd");
    return RP_OK;
}

extern "C" int rp_interest_pick_bwd(const float *dbest, const int32_t *kidx, int64_t B, int K, int D, float *dout,
                                    rp_stream_t stream) {
    RP_REQUIRE(dbest && kidx && dout, "interest_pick_bwd: null pointer");
    RP_REQUIRE(B >= 0 && K >= 1 && D >= 1 && B * K * D <= (int64_t)INT32_MAX * 256, "interest_pick_bwd: need B >= 0 and K, D >= 1");
    if (B == 0) return RP_OK;
    const int64_t total = B * K * D;
    hipLaunchKernelGGL(cap_pick_bwd_kernel, dim3((unsigned)rp_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, dbest, kidx,
                       total, K, D, dout);
    RP_LAUNCH_CHECK("interest_pick_bwd");
    return RP_OK;
}
