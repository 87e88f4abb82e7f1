// AFN's logarithmic transformation layer (ranking/afn.py:93-102) and its two-logit ensemble head (afn.py:81), gfx950.
//
//   x = log(max(|e|, 1e-5f))               [B,F,D]   e: the gather's rows, read in place at any row stride
//   y = BN1(x)                                        channel = field f, statistics over (b, d)
//   z[b,l,d] = sum_f W[l,f] y[b,f,d]        [B,L,D]   the only intermediate that is stored (L << F)
//   c = exp(z);  out = BN2(c)                         channel = neuron l, statistics over (b, d)
//
// Neither x, y nor c ever exists in global memory: the forward rebuilds nothing, the backward rebuilds y from the rows and
// c from z.  One thread owns one (sample, column) pair — M = B D "elements" — and walks the F fields of that column, so
// a wave reads runs of D consecutive floats.  W and the per-field / per-neuron constants sit in LDS (read as broadcasts);
// the only per-thread arrays are indexed by the compile-time neuron index (template <L>), so nothing goes to scratch.
// logf / expf are the accurate ones: the block is bound by its row traffic, not by them.
//
// Reductions (both BatchNorms' statistics, their backward sums, dW): a workgroup owns a run of `chunk` elements
// (ln_plan: at most 512 workgroups), leaves its partial in the workspace and a finishing launch adds the partials in a
// fixed order — 16 slices of every 16th partial, then the slices in order, as norm.hip's bn_finish_kernel does.  No
// atomics; the workspace depends on (F, L) only.  Variances are centred: a workgroup leaves (mean, M2) of its own
// elements and the finish merges the pairs (Chan et al.), never E[v^2] - E[v]^2.
#include "common.h"

#define LN_FMAX 64
#define LN_LMAX 8
#define LN_DMAX 256
#define LN_MAXBLK 512
#define LN_E 8                      // elements per thread and round of the parameter-gradient pass
#define LN_ROUND (256 * LN_E)
#define LN_THR 1e-5f                // the clamp: float32(1e-5), compared with >=

struct LnPlan {
    int64_t chunk;  // elements per partial workgroup (a multiple of LN_ROUND)
    int nblk;       // partial workgroups of every reduction over the M = B D elements
};

static LnPlan ln_plan(int64_t M) {
    LnPlan p;
    int64_t c = rp_cdiv(M, LN_MAXBLK);
    if (c < LN_ROUND) c = LN_ROUND;
    p.chunk = rp_cdiv(c, LN_ROUND) * LN_ROUND;
    p.nblk = (int)rp_cdiv(M, p.chunk);
    return p;
}

__device__ __forceinline__ float ln_logabs(float v) { return logf(fmaxf(fabsf(v), LN_THR)); }

// t = q D + rem for t < 2^23 (an offset inside one workgroup's chunk): a float reciprocal and one correction
__device__ __forceinline__ void ln_split(uint32_t t, int D, float invD, uint32_t &q, int &rem) {
    q = (uint32_t)((float)t * invD);
    int r = (int)t - (int)(q * (uint32_t)D);
    if (r < 0) {
        --q;
        r += D;
    } else if (r >= D) {
        ++q;
        r -= D;
    }
    rem = r;
}

// sums of v[0..K) over the 256 threads, the same in every thread; red: 4 K floats of LDS
template <int K>
__device__ __forceinline__ void ln_block_sum(float (&v)[K], float *red) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();  // (the previous use of red has been read)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// ---- BN1's batch statistics: partial[blk][f] = (mean, M2) of x over the workgroup's elements
__global__ __launch_bounds__(256) void ln_stat1_kernel(const float *__restrict__ x, int64_t ldx, int64_t M, int F, int D,
                                                       int64_t chunk, float *__restrict__ partial) {
    __shared__ float red[4];
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < M ? i0 + chunk : M;
    const uint32_t n = (uint32_t)(i1 - i0);
    const int64_t b0 = i0 / D;
    const uint32_t d0 = (uint32_t)(i0 - b0 * D);
    const float invD = 1.f / (float)D;
    const float *xb = x + b0 * ldx;
    for (int f = 0; f < F; ++f) {
        float s[1] = {0.f};
        for (uint32_t r = threadIdx.x; r < n; r += 256) {
            uint32_t q;
            int d;
            ln_split(r + d0, D, invD, q, d);
            s[0] += ln_logabs(xb[(int64_t)q * ldx + f * D + d]);
        }
        ln_block_sum<1>(s, red);
        const float mb = s[0] / (float)n;
        float m2[1] = {0.f};
        for (uint32_t r = threadIdx.x; r < n; r += 256) {
            uint32_t q;
            int d;
            ln_split(r + d0, D, invD, q, d);
            const float dl = ln_logabs(xb[(int64_t)q * ldx + f * D + d]) - mb;
            m2[0] += dl * dl;
        }
        ln_block_sum<1>(m2, red);
        if (threadIdx.x == 0) {
            partial[((int64_t)blockIdx.x * F + f) * 2 + 0] = mb;
            partial[((int64_t)blockIdx.x * F + f) * 2 + 1] = m2[0];
        }
    }
}

// merges partial[k][n] = (mean_k, M2_k) over n_k = min(chunk, M - k chunk) elements into mean[n], var[n] (biased).
// 16 channels x 16 slices per workgroup; slice s takes partials s, s + 16, ...; the slices combine in order.
__global__ __launch_bounds__(256) void ln_finish_stats_kernel(const float *__restrict__ partial, int nblk, int N, int64_t M,
                                                              int64_t chunk, float *__restrict__ mean,
                                                              float *__restrict__ var) {
    __shared__ float red[256];
    __shared__ float smean[16];
    const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + c;
    float a = 0.f;
    if (n < N)
        for (int k = sl; k < nblk; k += 16) {
            const int64_t rest = M - (int64_t)k * chunk;
            a += (float)(rest < chunk ? rest : chunk) * partial[((int64_t)k * N + n) * 2];
        }
    red[threadIdx.x] = a;
    __syncthreads();
    if (sl == 0) {
        for (int q = 1; q < 16; ++q) a += red[q * 16 + c];
        smean[c] = a / (float)M;
    }
    __syncthreads();
    const float mu = smean[c];
    float m2 = 0.f;
    if (n < N)
        for (int k = sl; k < nblk; k += 16) {
            const int64_t rest = M - (int64_t)k * chunk;
            const float dl = partial[((int64_t)k * N + n) * 2] - mu;
            m2 += partial[((int64_t)k * N + n) * 2 + 1] + (float)(rest < chunk ? rest : chunk) * dl * dl;
        }
    red[threadIdx.x] = m2;
    __syncthreads();
    if (sl != 0 || n >= N) return;
    for (int q = 1; q < 16; ++q) m2 += red[q * 16 + c];
    mean[n] = mu;
    var[n] = m2 / (float)M;
}

// sums[n] = sum_k partial[k][n] in the same fixed order; copied out in up to three segments (nA, nB, the rest)
__global__ __launch_bounds__(256) void ln_finish_sum_kernel(const float *__restrict__ partial, int nblk, int N,
                                                            float *__restrict__ sums, float *__restrict__ outA, int nA,
                                                            float *__restrict__ outB, int nB, float *__restrict__ outC) {
    __shared__ float red[256];
    const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + c;
    float a = 0.f;
    if (n < N)
        for (int k = sl; k < nblk; k += 16) a += partial[(int64_t)k * N + n];
    red[threadIdx.x] = a;
    __syncthreads();
    if (sl != 0 || n >= N) return;
    for (int q = 1; q < 16; ++q) a += red[q * 16 + c];
    if (sums != nullptr) sums[n] = a;
    if (n < nA) {
        if (outA != nullptr) outA[n] = a;
    } else if (n < nA + nB) {
        if (outB != nullptr) outB[n - nA] = a;
    } else if (outC != nullptr) {
        outC[n - nA - nB] = a;
    }
}

// ---- forward: z for every element, then  TRAIN: partial[blk][l] = (mean, M2) of c = exp(z)
//                                          else : out = BN2(c) with the given (running) statistics
template <int L, bool TRAIN>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ W,
                                                     const float *__restrict__ gamma1, const float *__restrict__ beta1,
                                                     const float *__restrict__ mean1, const float *__restrict__ var1,
                                                     float eps1, const float *__restrict__ gamma2,
                                                     const float *__restrict__ beta2, const float *__restrict__ mean2,
                                                     const float *__restrict__ var2, float eps2, float *__restrict__ z,
                                                     float *__restrict__ out, int64_t ldo, int64_t M, int F, int D,
                                                     int64_t chunk, float *__restrict__ partial) {
    __shared__ float sW[LN_FMAX * L];  // [f][l]
    __shared__ float smu[LN_FMAX], sk[LN_FMAX], sbe[LN_FMAX];
    __shared__ float red[4 * L];
    for (int t = threadIdx.x; t < F * L; t += 256) {
        const int f = t / L, l = t - f * L;
        sW[t] = W[l * F + f];
    }
    for (int f = threadIdx.x; f < F; f += 256) {
        smu[f] = mean1[f];
        sk[f] = gamma1[f] * (1.f / sqrtf(var1[f] + eps1));
        sbe[f] = beta1[f];
    }
    float mu2[L], k2[L], be2[L];
    if (!TRAIN) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            mu2[l] = mean2[l];
            k2[l] = gamma2[l] * (1.f / sqrtf(var2[l] + eps2));
            be2[l] = beta2[l];
        }
    }
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < M ? i0 + chunk : M;
    const uint32_t n = (uint32_t)(i1 - i0);
    const int64_t b0 = i0 / D;
    const uint32_t d0 = (uint32_t)(i0 - b0 * D);
    const float invD = 1.f / (float)D;
    const int64_t ldz = (int64_t)L * D;
    float s[L];
#pragma unroll
    for (int l = 0; l < L; ++l) s[l] = 0.f;
    for (uint32_t r = threadIdx.x; r < n; r += 256) {
        uint32_t q;
        int d;
        ln_split(r + d0, D, invD, q, d);
        const float *xp = x + (b0 + q) * ldx + d;
        float acc[L];
#pragma unroll
        for (int l = 0; l < L; ++l) acc[l] = 0.f;
        for (int f = 0; f < F; ++f) {
            const float y = (ln_logabs(xp[f * D]) - smu[f]) * sk[f] + sbe[f];
#pragma unroll
            for (int l = 0; l < L; ++l) acc[l] = __builtin_fmaf(sW[f * L + l], y, acc[l]);
        }
        float *zp = z + (b0 + q) * ldz + d;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            zp[l * D] = acc[l];
            const float c = expf(acc[l]);
            if (TRAIN) s[l] += c;
            else out[(b0 + q) * ldo + l * D + d] = (c - mu2[l]) * k2[l] + be2[l];
        }
    }
    if (!TRAIN) return;
    ln_block_sum<L>(s, red);
    float m2[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        s[l] = s[l] / (float)n;
        m2[l] = 0.f;
    }
    for (uint32_t r = threadIdx.x; r < n; r += 256) {  // (this thread's own z, written above)
        uint32_t q;
        int d;
        ln_split(r + d0, D, invD, q, d);
        const float *zp = z + (b0 + q) * ldz + d;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float dl = expf(zp[l * D]) - s[l];
            m2[l] += dl * dl;
        }
    }
    ln_block_sum<L>(m2, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            partial[((int64_t)blockIdx.x * L + l) * 2 + 0] = s[l];
            partial[((int64_t)blockIdx.x * L + l) * 2 + 1] = m2[l];
        }
    }
}

// out = BN2(exp(z)) with the finished batch statistics; blockIdx.y = l
__global__ __launch_bounds__(256) void ln_apply_kernel(const float *__restrict__ z, const float *__restrict__ gamma2,
                                                       const float *__restrict__ beta2, const float *__restrict__ mean2,
                                                       const float *__restrict__ var2, float eps2, float *__restrict__ out,
                                                       int64_t ldo, int64_t M, int L, int D) {
    const int l = blockIdx.y;
    const float mu = mean2[l], k = gamma2[l] * (1.f / sqrtf(var2[l] + eps2)), be = beta2[l];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int64_t b = (int64_t)((uint32_t)i / (uint32_t)D);
    const int d = (int)(i - b * D);
    out[b * ldo + l * D + d] = (expf(z[(b * L + l) * D + d]) - mu) * k + be;
}

// ---- backward, first sums: partial[blk][l] = sum g, partial[blk][L + l] = sum g chat   (dbeta2, dgamma2)
__global__ __launch_bounds__(256) void ln_bwd_sums2_kernel(const float *__restrict__ dout, int64_t lddo,
                                                           const float *__restrict__ z, const float *__restrict__ mean2,
                                                           const float *__restrict__ var2, float eps2, int64_t M, int L, int D,
                                                           int64_t chunk, float *__restrict__ partial) {
    __shared__ float red[8];
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < M ? i0 + chunk : M;
    const uint32_t n = (uint32_t)(i1 - i0);
    const int64_t b0 = i0 / D;
    const uint32_t d0 = (uint32_t)(i0 - b0 * D);
    const float invD = 1.f / (float)D;
    const int64_t ldz = (int64_t)L * D;
    for (int l = 0; l < L; ++l) {
        const float mu = mean2[l], rs = 1.f / sqrtf(var2[l] + eps2);
        float s[2] = {0.f, 0.f};
        for (uint32_t r = threadIdx.x; r < n; r += 256) {
            uint32_t q;
            int d;
            ln_split(r + d0, D, invD, q, d);
            const float g = dout[(b0 + q) * lddo + l * D + d];
            const float ch = (expf(z[(b0 + q) * ldz + l * D + d]) - mu) * rs;
            s[0] += g;
            s[1] = __builtin_fmaf(g, ch, s[1]);
        }
        ln_block_sum<2>(s, red);
        if (threadIdx.x == 0) {
            partial[(int64_t)blockIdx.x * 2 * L + l] = s[0];
            partial[(int64_t)blockIdx.x * 2 * L + L + l] = s[1];
        }
    }
}

// the per-neuron constants of BN2's backward in LDS: c2[0] mean, [1] rstd, [2] gamma rstd, [3] mean g, [4] mean g chat
template <int L>
__device__ __forceinline__ void ln_stage_bn2(float (*c2)[L], const float *gamma2, const float *mean2, const float *var2,
                                             float eps2, const float *sums2, int train, float invM) {
    if (threadIdx.x < L) {
        const int l = threadIdx.x;
        const float rs = 1.f / sqrtf(var2[l] + eps2);
        c2[0][l] = mean2[l];
        c2[1][l] = rs;
        c2[2][l] = gamma2[l] * rs;
        c2[3][l] = train ? sums2[l] * invM : 0.f;
        c2[4][l] = train ? sums2[L + l] * invM : 0.f;
    }
}

// dz[l] = dc c of one element, dc = BN2'(g)
template <int L>
__device__ __forceinline__ void ln_dz(float (&dz)[L], const float *gp, const float *zp, int D, float (*c2)[L]) {
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const float c = expf(zp[l * D]);
        const float ch = (c - c2[0][l]) * c2[1][l];
        dz[l] = c2[2][l] * (gp[l * D] - c2[3][l] - ch * c2[4][l]) * c;
    }
}

// ---- backward, parameter sums: partial[blk][k][f], k < L: sum dz_l y_f (dW[l,f]); k = L: sum dy_f; k = L + 1: sum dy_f yhat_f
template <int L>
__global__ __launch_bounds__(256) void ln_bwd_params_kernel(const float *__restrict__ dout, int64_t lddo,
                                                            const float *__restrict__ x, int64_t ldx,
                                                            const float *__restrict__ z, const float *__restrict__ W,
                                                            const float *__restrict__ gamma1, const float *__restrict__ beta1,
                                                            const float *__restrict__ mean1, const float *__restrict__ var1,
                                                            float eps1, const float *__restrict__ gamma2,
                                                            const float *__restrict__ mean2, const float *__restrict__ var2,
                                                            float eps2, const float *__restrict__ sums2, int train, int64_t M,
                                                            int F, int D, int64_t chunk, float *__restrict__ partial) {
    constexpr int K = L + 2;
    __shared__ float sW[LN_FMAX * L];
    __shared__ float smu[LN_FMAX], srs[LN_FMAX], sg[LN_FMAX], sbe[LN_FMAX];
    __shared__ float c2[5][L];
    __shared__ float sacc[K * LN_FMAX];
    __shared__ float red[4 * K];
    for (int t = threadIdx.x; t < F * L; t += 256) {
        const int f = t / L, l = t - f * L;
        sW[t] = W[l * F + f];
    }
    for (int f = threadIdx.x; f < F; f += 256) {
        smu[f] = mean1[f];
        srs[f] = 1.f / sqrtf(var1[f] + eps1);
        sg[f] = gamma1[f];
        sbe[f] = beta1[f];
    }
    for (int t = threadIdx.x; t < K * LN_FMAX; t += 256) sacc[t] = 0.f;
    ln_stage_bn2<L>(c2, gamma2, mean2, var2, eps2, sums2, train, 1.f / (float)M);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < M ? i0 + chunk : M;
    const uint32_t n = (uint32_t)(i1 - i0);
    const int64_t b0 = i0 / D;
    const uint32_t d0 = (uint32_t)(i0 - b0 * D);
    const float invD = 1.f / (float)D;
    const int64_t ldz = (int64_t)L * D;
    for (uint32_t r0 = 0; r0 < n; r0 += LN_ROUND) {
        float dz[LN_E][L];
        int64_t off[LN_E];  // the element's offset in the rows, or -1 past the end
#pragma unroll
        for (int e = 0; e < LN_E; ++e) {
            const uint32_t r = r0 + e * 256 + threadIdx.x;
            off[e] = -1;
#pragma unroll
            for (int l = 0; l < L; ++l) dz[e][l] = 0.f;
            if (r < n) {
                uint32_t q;
                int d;
                ln_split(r + d0, D, invD, q, d);
                off[e] = (b0 + q) * ldx + d;
                ln_dz<L>(dz[e], dout + (b0 + q) * lddo + d, z + (b0 + q) * ldz + d, D, c2);
            }
        }
        for (int f = 0; f < F; ++f) {
            float a[K];
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] = 0.f;
            const float mu = smu[f], rs = srs[f], g1 = sg[f], b1 = sbe[f];
#pragma unroll
            for (int e = 0; e < LN_E; ++e) {
                if (off[e] < 0) continue;
                const float yh = (ln_logabs(x[off[e] + f * D]) - mu) * rs;
                const float y = yh * g1 + b1;
                float dy = 0.f;
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    dy = __builtin_fmaf(sW[f * L + l], dz[e][l], dy);
                    a[l] = __builtin_fmaf(dz[e][l], y, a[l]);
                }
                a[L] += dy;
                a[L + 1] = __builtin_fmaf(dy, yh, a[L + 1]);
            }
            ln_block_sum<K>(a, red);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) sacc[k * LN_FMAX + f] += a[k];
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K * F; t += 256) {
        const int k = t / F, f = t - k * F;
        partial[(int64_t)blockIdx.x * K * F + t] = sacc[k * LN_FMAX + f];
    }
}

// ---- backward, input gradient: dx = BN1'(W^T dz) / e where |e| >= 1e-5f, else 0
template <int L>
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(const float *__restrict__ dout, int64_t lddo,
                                                        const float *__restrict__ x, int64_t ldx, const float *__restrict__ z,
                                                        const float *__restrict__ W, const float *__restrict__ gamma1,
                                                        const float *__restrict__ mean1, const float *__restrict__ var1,
                                                        float eps1, const float *__restrict__ gamma2,
                                                        const float *__restrict__ mean2, const float *__restrict__ var2,
                                                        float eps2, const float *__restrict__ sums2,
                                                        const float *__restrict__ sums1, int train, float *__restrict__ dx,
                                                        int64_t lddx, int64_t M, int F, int D) {
    __shared__ float sW[LN_FMAX * L];
    __shared__ float smu[LN_FMAX], srs[LN_FMAX], sk[LN_FMAX], smd[LN_FMAX], smdy[LN_FMAX];
    __shared__ float c2[5][L];
    const float invM = 1.f / (float)M;
    for (int t = threadIdx.x; t < F * L; t += 256) {
        const int f = t / L, l = t - f * L;
        sW[t] = W[l * F + f];
    }
    for (int f = threadIdx.x; f < F; f += 256) {
        const float rs = 1.f / sqrtf(var1[f] + eps1);
        smu[f] = mean1[f];
        srs[f] = rs;
        sk[f] = gamma1[f] * rs;
        smd[f] = train ? sums1[L * F + f] * invM : 0.f;
        smdy[f] = train ? sums1[(L + 1) * F + f] * invM : 0.f;
    }
    ln_stage_bn2<L>(c2, gamma2, mean2, var2, eps2, sums2, train, invM);
    __syncthreads();
    const int64_t ldz = (int64_t)L * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t b = (int64_t)((uint32_t)i / (uint32_t)D);
        const int d = (int)(i - b * D);
        float dz[L];
        ln_dz<L>(dz, dout + b * lddo + d, z + b * ldz + d, D, c2);
        const float *xp = x + b * ldx + d;
        float *dp = dx + b * lddx + d;
        for (int f = 0; f < F; ++f) {
            const float v = xp[f * D];
            const float yh = (ln_logabs(v) - smu[f]) * srs[f];
            float dy = 0.f;
#pragma unroll
            for (int l = 0; l < L; ++l) dy = __builtin_fmaf(sW[f * L + l], dz[l], dy);
            const float t = sk[f] * (dy - smd[f] - yh * smdy[f]);
            dp[f * D] = fabsf(v) >= LN_THR ? t / v : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int rp_lognet_fits(int F, int D, int L) {
    return F >= 1 && F <= LN_FMAX && D >= 1 && D <= LN_DMAX && L >= 1 && L <= LN_LMAX;
}

extern "C" int rp_lognet_plan(int64_t B, int D, int *nblk, int64_t *chunk) {
    RP_REQUIRE(B >= 1 && D >= 1 && D <= LN_DMAX && B * D < ((int64_t)1 << 31), "lognet_plan: bad argument");
    const LnPlan p = ln_plan(B * D);
    if (nblk) *nblk = p.nblk;
    if (chunk) *chunk = p.chunk;
    return RP_OK;
}

// partials [512][max(F (L + 2), 2 L)] | sums1 [F (L + 2)] | sums2 [2 L]
extern "C" int rp_lognet_workspace_bytes(int F, int L, size_t *bytes) {
    RP_REQUIRE(bytes && F >= 1 && L >= 1, "lognet_workspace_bytes: bad argument");
    const size_t n1 = (size_t)F * (L + 2), n2 = 2 * (size_t)L;
    *bytes = (LN_MAXBLK * (n1 > n2 ? n1 : n2) + n1 + n2) * sizeof(float) + 256;
    return RP_OK;
}

struct LnWs {
    float *P, *sums1, *sums2;
};

static LnWs ln_ws(void *workspace, int F, int L) {
    LnWs w;
    const size_t n1 = (size_t)F * (L + 2), n2 = 2 * (size_t)L;
    w.P = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    w.sums1 = w.P + LN_MAXBLK * (n1 > n2 ? n1 : n2);
    w.sums2 = w.sums1 + n1;
    return w;
}

#define LN_DISPATCH(L, CALL)     \
    switch (L) {                 \
        case 1: CALL(1); break;  \
        case 2: CALL(2); break;  \
        case 3: CALL(3); break;  \
        case 4: CALL(4); break;  \
        case 5: CALL(5); break;  \
        case 6: CALL(6); break;  \
        case 7: CALL(7); break;  \
        default: CALL(8); break; \
    }

extern "C" int rp_lognet_fwd(const float *x, int64_t ldx, const float *W, const float *gamma1, const float *beta1,
                             float *mean1, float *var1, float eps1, const float *gamma2, const float *beta2, float *mean2,
                             float *var2, float eps2, float *z, float *out, int64_t ldo, int64_t B, int F, int D, int L,
                             int train, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(x && W && gamma1 && beta1 && mean1 && var1 && gamma2 && beta2 && mean2 && var2 && z && out,
               "lognet_fwd: null pointer");
    RP_REQUIRE(B >= 0 && F >= 1 && D >= 1 && L >= 1, "lognet_fwd: bad shape");
    if (!rp_lognet_fits(F, D, L)) return rp_fail(RP_ERR_UNSUPPORTED, "lognet_fwd: F=%d D=%d L=%d outside rp_lognet_fits", F, D, L);
    RP_REQUIRE(ldx >= (int64_t)F * D && ldo >= (int64_t)L * D && B * D < ((int64_t)1 << 31), "lognet_fwd: bad row stride or batch");
    if (B == 0) return RP_OK;
    size_t need = 0;
    rp_lognet_workspace_bytes(F, L, &need);
    RP_REQUIRE(!train || (workspace && workspace_bytes >= need), "lognet_fwd: workspace %zu < %zu", workspace_bytes, need);
    const int64_t M = B * D;
    const LnPlan p = ln_plan(M);
    hipStream_t s = (hipStream_t)stream;
    if (train) {
        const LnWs w = ln_ws(workspace, F, L);
        hipLaunchKernelGGL(ln_stat1_kernel, dim3((unsigned)p.nblk), dim3(256), 0, s, x, ldx, M, F, D, p.chunk, w.P);
        RP_LAUNCH_CHECK("lognet log statistics");
        hipLaunchKernelGGL(ln_finish_stats_kernel, dim3((unsigned)rp_cdiv(F, 16)), dim3(256), 0, s, w.P, p.nblk, F, M, p.chunk,
                           mean1, var1);
        RP_LAUNCH_CHECK("lognet log statistics finish");
#define CALL(LL)                                                                                                               \
    hipLaunchKernelGGL((ln_fwd_kernel<LL, true>), dim3((unsigned)p.nblk), dim3(256), 0, s, x, ldx, W, gamma1, beta1, mean1, var1, \
                       eps1, gamma2, beta2, mean2, var2, eps2, z, out, ldo, M, F, D, p.chunk, w.P)
        LN_DISPATCH(L, CALL)
#undef CALL
        RP_LAUNCH_CHECK("lognet z");
        hipLaunchKernelGGL(ln_finish_stats_kernel, dim3(1), dim3(256), 0, s, w.P, p.nblk, L, M, p.chunk, mean2, var2);
        RP_LAUNCH_CHECK("lognet exp statistics finish");
        hipLaunchKernelGGL(ln_apply_kernel, dim3((unsigned)rp_cdiv(M, 256), (unsigned)L), dim3(256), 0, s, z, gamma2, beta2,
                           mean2, var2, eps2, out, ldo, M, L, D);
        RP_LAUNCH_CHECK("lognet apply");
    } else {
#define CALL(LL)                                                                                                                \
    hipLaunchKernelGGL((ln_fwd_kernel<LL, false>), dim3((unsigned)p.nblk), dim3(256), 0, s, x, ldx, W, gamma1, beta1, mean1, var1, \
                       eps1, gamma2, beta2, mean2, var2, eps2, z, out, ldo, M, F, D, p.chunk, nullptr)
        LN_DISPATCH(L, CALL)
#undef CALL
        RP_LAUNCH_CHECK("lognet fwd");
    }
    return RP_OK;
}

extern "C" int rp_lognet_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *z, const float *W,
                             const float *gamma1, const float *beta1, const float *mean1, const float *var1, float eps1,
                             const float *gamma2, const float *mean2, const float *var2, float eps2, float *dx, int64_t lddx,
                             float *dW, float *dgamma1, float *dbeta1, float *dgamma2, float *dbeta2, int64_t B, int F, int D,
                             int L, int train, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(dout && x && z && W && gamma1 && beta1 && mean1 && var1 && gamma2 && mean2 && var2 && dx && dW && dgamma1 &&
                   dbeta1 && dgamma2 && dbeta2 && workspace, "lognet_bwd: null pointer");
    RP_REQUIRE(B >= 0 && F >= 1 && D >= 1 && L >= 1, "lognet_bwd: bad shape");
    if (!rp_lognet_fits(F, D, L)) return rp_fail(RP_ERR_UNSUPPORTED, "lognet_bwd: F=%d D=%d L=%d outside rp_lognet_fits", F, D, L);
    RP_REQUIRE(ldx >= (int64_t)F * D && lddx >= (int64_t)F * D && lddo >= (int64_t)L * D && B * D < ((int64_t)1 << 31),
               "lognet_bwd: bad row stride or batch");
    if (B == 0) return RP_OK;
    size_t need = 0;
    rp_lognet_workspace_bytes(F, L, &need);
    RP_REQUIRE(workspace_bytes >= need, "lognet_bwd: workspace %zu < %zu", workspace_bytes, need);
    const int64_t M = B * D;
    const LnPlan p = ln_plan(M);
    const LnWs w = ln_ws(workspace, F, L);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ln_bwd_sums2_kernel, dim3((unsigned)p.nblk), dim3(256), 0, s, dout, lddo, z, mean2, var2, eps2, M, L, D,
                       p.chunk, w.P);
    RP_LAUNCH_CHECK("lognet bwd exp sums");
    hipLaunchKernelGGL(ln_finish_sum_kernel, dim3(1), dim3(256), 0, s, w.P, p.nblk, 2 * L, w.sums2, dbeta2, L, dgamma2, L,
                       nullptr);
    RP_LAUNCH_CHECK("lognet bwd exp sums finish");
#define CALL(LL)                                                                                                              \
    hipLaunchKernelGGL((ln_bwd_params_kernel<LL>), dim3((unsigned)p.nblk), dim3(256), 0, s, dout, lddo, x, ldx, z, W, gamma1, \
                       beta1, mean1, var1, eps1, gamma2, mean2, var2, eps2, w.sums2, train, M, F, D, p.chunk, w.P)
    LN_DISPATCH(L, CALL)
#undef CALL
    RP_LAUNCH_CHECK("lognet bwd parameter sums");
    const int n1 = F * (L + 2);
    hipLaunchKernelGGL(ln_finish_sum_kernel, dim3((unsigned)rp_cdiv(n1, 16)), dim3(256), 0, s, w.P, p.nblk, n1, w.sums1, dW,
                       L * F, dbeta1, F, dgamma1);
    RP_LAUNCH_CHECK("lognet bwd parameter sums finish");
    int64_t gx = rp_cdiv(M, 256);
    if (gx > 8192) gx = 8192;
#define CALL(LL)                                                                                                           \
    hipLaunchKernelGGL((ln_bwd_dx_kernel<LL>), dim3((unsigned)gx), dim3(256), 0, s, dout, lddo, x, ldx, z, W, gamma1, mean1, \
                       var1, eps1, gamma2, mean2, var2, eps2, w.sums2, w.sums1, train, dx, lddx, M, F, D)
    LN_DISPATCH(L, CALL)
#undef CALL
    RP_LAUNCH_CHECK("lognet bwd dx");
    return RP_OK;
}

// ------------------------------------------------------------------------------------------------ the ensemble head
// afn.py:81  fc(cat[a, d]):  z[b] = w[0] a[b] + w[1] d[b] + bias[0];  the sigmoid and the loss are rp_sigmoid_bce_*.
__global__ __launch_bounds__(256) void pair_fc_fwd_kernel(const float *__restrict__ a, const float *__restrict__ d,
                                                          const float *__restrict__ w, const float *__restrict__ bias,
                                                          float *__restrict__ z, int64_t B) {
    const float w0 = w[0], w1 = w[1], b0 = bias[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256)
        z[i] = __builtin_fmaf(w1, d[i], __builtin_fmaf(w0, a[i], b0));
}

// da = w[0] dz, dd = w[1] dz;  partial[blk] = (sum dz a, sum dz d, sum dz) over the workgroup's run of samples
__global__ __launch_bounds__(256) void pair_fc_bwd_kernel(const float *__restrict__ dz, const float *__restrict__ a,
                                                          const float *__restrict__ d, const float *__restrict__ w,
                                                          float *__restrict__ da, float *__restrict__ dd, int64_t B,
                                                          int64_t chunk, float *__restrict__ partial) {
    __shared__ float red[12];
    const float w0 = w[0], w1 = w[1];
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < B ? i0 + chunk : B;
    float s[3] = {0.f, 0.f, 0.f};
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float g = dz[i];
        da[i] = w0 * g;
        dd[i] = w1 * g;
        s[0] = __builtin_fmaf(g, a[i], s[0]);
        s[1] = __builtin_fmaf(g, d[i], s[1]);
        s[2] += g;
    }
    ln_block_sum<3>(s, red);
    if (threadIdx.x == 0) {
        partial[(int64_t)blockIdx.x * 3 + 0] = s[0];
        partial[(int64_t)blockIdx.x * 3 + 1] = s[1];
        partial[(int64_t)blockIdx.x * 3 + 2] = s[2];
    }
}

static LnPlan pair_fc_plan(int64_t B) {
    LnPlan p;
    int64_t c = rp_cdiv(B, LN_MAXBLK);
    if (c < 1024) c = 1024;
    p.chunk = rp_cdiv(c, 256) * 256;
    p.nblk = (int)rp_cdiv(B, p.chunk);
    return p;
}

extern "C" int rp_pair_fc_partials(int64_t B) { return B >= 1 ? 3 * pair_fc_plan(B).nblk : 3; }

extern "C" int rp_pair_fc_fwd(const float *a, const float *d, const float *w, const float *bias, float *z, int64_t B,
                              rp_stream_t stream) {
    RP_REQUIRE(a && d && w && bias && z && B >= 0, "pair_fc_fwd: bad argument");
    if (B == 0) return RP_OK;
    int64_t gx = rp_cdiv(B, 256);
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(pair_fc_fwd_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, a, d, w, bias, z, B);
    RP_LAUNCH_CHECK("pair_fc_fwd");
    return RP_OK;
}

extern "C" int rp_pair_fc_bwd(const float *dz, const float *a, const float *d, const float *w, float *da, float *dd, float *dw,
                              float *dbias, float *partial, int64_t B, rp_stream_t stream) {
    RP_REQUIRE(dz && a && d && w && da && dd && dw && dbias && partial && B >= 1, "pair_fc_bwd: bad argument");
    const LnPlan p = pair_fc_plan(B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pair_fc_bwd_kernel, dim3((unsigned)p.nblk), dim3(256), 0, s, dz, a, d, w, da, dd, B, p.chunk, partial);
    RP_LAUNCH_CHECK("pair_fc_bwd");
    hipLaunchKernelGGL(ln_finish_sum_kernel, dim3(1), dim3(256), 0, s, partial, p.nblk, 3, nullptr, dw, 2, dbias, 1, nullptr);
    RP_LAUNCH_CHECK("pair_fc_bwd finish");
    return RP_OK;
}
