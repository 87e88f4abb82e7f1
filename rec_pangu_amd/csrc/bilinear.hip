// FiBiNet's SENET + bilinear interaction (layers/interaction.py:55-81, :238-251; ranking/fibinet.py:58-68) as one launch
// forward and three kinds of launch backward, fp32, gfx950.
//
// rp_bilinear_*  reference:  Z = mean_d E,  A = relu(W2 relu(W1 Z)),  V = E * A[..., None];  for the pair p = (i, j), i < j, in
//                itertools.combinations order  T(E)[b, p, :] = (W_w(p) E[b, i, :]) * E[b, j, :];  the MLP input is
//                cat(flatten(cat(T(E), T(V), dim=1)), dense).  A is a scalar per (sample, field), so
//                    T(V)[b, p, :] = A[b, i] A[b, j] T(E)[b, p, :]:
//                the matrix-vector product is formed ONCE per pair, the second branch is s = A_i A_j times the first, and V
//                is never formed.  R = 0 means no SENET: one branch (the stand-alone BilinearInteractionLayer).
//
// Why vector FMA and not the matrix core.  Per pair the forward does 2 D^2 flops and stores 2 D floats: D / 4 = 8 flop per
// stored byte at D = 32, below the fp32 vector ridge of the part, so the forward is bound by the 2 P D floats it writes per
// sample.  What matters is weight reuse: W_p must not be fetched per sample.
//
// forward   a workgroup (256 threads) owns a tile of TB samples (the largest power of two <= 32 whose working set is within
//           64 KiB of LDS: 16 at F = 26, D = 32).  The tile's embedding columns are read from the caller's rows in place
//           (row stride, no copy) into LDS as [sample][F D]; Z, the hidden layer and A are computed from that tile in a
//           prologue.  Thread (g, d) = (tid / D, tid % D) then takes pair p = pass 256 / D + g, loads row d of W_p into D
//           registers ONCE and applies it to every sample of the tile: E_i is read as float4 with one address per pair (an
//           LDS broadcast), E_j[d] with consecutive lanes on consecutive banks; the sample stride never separates two lanes
//           of one instruction, so it needs no padding.  The wave's stores are 64 consecutive floats of the row.  grid.y
//           splits the passes when the batch alone gives too few workgroups.  Nothing but the MLP input is stored.
// backward  the batch is walked in chunks of BIL_CHUNK samples, so that A can be handed from the sample-major to the
//           pair-major launch through a scratch of BIL_CHUNK x F floats: the workspace does not depend on B.
//   rows    sample-major: the D threads of one sample sit in one wave (a tile is 256 / D samples).  E and the dE
//           accumulators of the tile are in LDS, thread (sample, d) being the only one that touches dE[sample, :, d]; W_p is
//           staged for the whole workgroup, double buffered, with row stride D + 4 floats (float4 row reads of 16 lanes fall
//           on 16 different 16-byte slots since D / 4 + 1 is odd; column reads W[k][d] have consecutive lanes on consecutive
//           banks).  Per pair: U = W E_i (recomputed), T = U * E_j, g = g_p + s g_q, ds = sum_d g_q T (a fixed butterfly
//           over the sample's lanes), dA_i += ds A_j, dA_j += ds A_i, dE_j += g U, dU = g E_j, dE_i += W^T dU (dU_k by a
//           lane shuffle).  Then dA goes through the two ReLUs (gradient 0 at a pre-activation <= 0) to the workgroup's dW2 /
//           dW1 accumulators and to dZ, and dE + dZ / D leaves as dx (written or added).  A workgroup walks its tiles in
//           order and stores its accumulators as ITS partial.
//   wgrad   pair-major: workgroup (p, slice) forms dU = g * E_j for 64 samples at a time in LDS and accumulates dU (x) E_i
//           over its slice in registers (thread: column k, rows d, d + 256 / D, ...), samples in order.
//   finish  one thread per parameter element: slices in order, then the pairs that share the weight in pair order; SENET
//           partials in workgroup order.
// No floating-point atomics anywhere: bit-identical from run to run.  A later chunk adds its sums to the slots of the first
// one (every slot has one owner per launch).
#include "common.h"

#define BIL_T 256
#define BIL_MAXF 40
#define BIL_CHUNK 16384      // samples per backward pass (rows of the A scratch)
#define BIL_SLICES 8         // batch slices of a chunk in the pair-major launch
#define BIL_MIN_SLICE 32     // samples of a slice at least
#define BIL_BWD_BLOCKS 512   // workgroups of the sample-major launch at most (= SENET partials)
#define BIL_WTILE 64         // samples staged at a time by the pair-major launch
#define BIL_FWD_LDS (64 * 1024)
#define BIL_BWD_LDS (152 * 1024)

struct BilGeom {
    int F, D, R, P, NW;
};

static bool bil_geom(int F, int D, int R, int type, BilGeom *g) {
    if (F < 2 || F > BIL_MAXF || (D != 8 && D != 16 && D != 32 && D != 64) || R < 0 || R > F) return false;
    if (type != RP_BILINEAR_ALL && type != RP_BILINEAR_EACH && type != RP_BILINEAR_INTERACTION) return false;
    g->F = F, g->D = D, g->R = R, g->P = F * (F - 1) / 2;
    g->NW = type == RP_BILINEAR_ALL ? 1 : type == RP_BILINEAR_EACH ? F : g->P;
    return true;
}

// LDS floats of the forward for a tile of tb samples: E, Z, hidden, A, the (i, j) bytes of the pairs
static size_t bil_fwd_lds_bytes(const BilGeom &g, int tb) {
    const int r1 = g.R > 0 ? g.R : 1;
    return (size_t)(tb * g.F * g.D + tb * (2 * g.F + r1)) * sizeof(float) + (size_t)((2 * g.P + 15) / 16 * 16);
}
static int bil_fwd_tile(const BilGeom &g) {
    int tb = 32;
    while (tb > 1 && bil_fwd_lds_bytes(g, tb) > BIL_FWD_LDS) tb >>= 1;
    return tb;
}
// sample-major backward: E, dE, 2 W buffers, Z, hidden, A, dA, dhidden, dZ, the SENET accumulators, the pair bytes
static size_t bil_bwd_lds_bytes(const BilGeom &g) {
    const int tb = BIL_T / g.D, r1 = g.R > 0 ? g.R : 1;
    return (size_t)(2 * tb * g.F * g.D + 2 * g.D * (g.D + 4) + tb * (4 * g.F + 2 * r1) + 2 * g.R * g.F) * sizeof(float) +
           (size_t)((2 * g.P + 15) / 16 * 16);
}

__device__ __forceinline__ void bil_pairs(int F, unsigned char *__restrict__ pi, unsigned char *__restrict__ pj) {
    for (int i = threadIdx.x; i < F - 1; i += BIL_T) {
        const int base = i * (2 * F - i - 1) / 2;
        for (int j = i + 1; j < F; ++j) pi[base + j - i - 1] = (unsigned char)i, pj[base + j - i - 1] = (unsigned char)j;
    }
}

// rows [b0, b0 + nb) of x, columns [0, FD), into Et [tb][FD]; the rows behind nb are zero
__device__ __forceinline__ void bil_stage(const float *__restrict__ x, int64_t ldx, int64_t b0, int nb, int tb, int FD,
                                          float *__restrict__ Et) {
    for (int idx = threadIdx.x; idx < tb * FD; idx += BIL_T) {
        const int b = idx / FD, c = idx - b * FD;
        Et[idx] = b < nb ? x[(b0 + b) * ldx + c] : 0.f;
    }
}

// Z = mean_d E, H = relu(W1 Z), A = relu(W2 H) of the tile in Et; Et must be visible; ends with a barrier
__device__ __forceinline__ void bil_senet(const float *__restrict__ Et, int tb, int F, int D, int R,
                                          const float *__restrict__ W1, const float *__restrict__ W2, float *__restrict__ Zs,
                                          float *__restrict__ Hs, float *__restrict__ As) {
    const float inv = 1.f / (float)D;
    for (int t = threadIdx.x; t < tb * F; t += BIL_T) {
        const float *e = Et + (size_t)t * D;  // (t = b F + f: the field's D floats)
        float s = 0.f;
        for (int d = 0; d < D; ++d) s += e[d];
        Zs[t] = s * inv;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tb * R; t += BIL_T) {
        const int b = t / R, r = t - b * R;
        float s = 0.f;
        for (int f = 0; f < F; ++f) s += W1[r * F + f] * Zs[b * F + f];
        Hs[t] = s > 0.f ? s : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tb * F; t += BIL_T) {
        const int b = t / F, f = t - b * F;
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += W2[f * R + r] * Hs[b * R + r];
        As[t] = s > 0.f ? s : 0.f;
    }
    __syncthreads();
}

__device__ __forceinline__ int bil_wclamp(int w, int NW) { return w < 0 ? 0 : (w >= NW ? NW - 1 : w); }

template <int D>
__global__ __launch_bounds__(BIL_T) void bil_fwd_kernel(const float *__restrict__ x, int64_t ldx,
                                                        const float *__restrict__ W1, const float *__restrict__ W2,
                                                        const float *const *__restrict__ wtab,
                                                        const int *__restrict__ wmap, float *__restrict__ out, int64_t ldo,
                                                        int64_t B, int ND, int tb, BilGeom g) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    const int F = g.F, R = g.R, P = g.P, FD = F * D, r1 = R > 0 ? R : 1;
    float *Et = bil_lds, *Zs = Et + tb * FD, *Hs = Zs + tb * F, *As = Hs + tb * r1;
    unsigned char *pi = reinterpret_cast<unsigned char *>(As + tb * F), *pj = pi + P;
    const int64_t b0 = (int64_t)blockIdx.x * tb;
    const int nb = B - b0 < tb ? (int)(B - b0) : tb;
    bil_pairs(F, pi, pj);
    bil_stage(x, ldx, b0, nb, tb, FD, Et);
    const int64_t obase = (int64_t)(R > 0 ? 2 : 1) * P * D;
    if (blockIdx.y == 0)  // the dense columns behind the branches
        for (int idx = threadIdx.x; idx < nb * ND; idx += BIL_T) {
            const int b = idx / ND, c = idx - b * ND;
            out[(b0 + b) * ldo + obase + c] = x[(b0 + b) * ldx + FD + c];
        }
    __syncthreads();
    if (R > 0) bil_senet(Et, tb, F, D, R, W1, W2, Zs, Hs, As);
    constexpr int G = BIL_T / D;
    const int grp = threadIdx.x / D, d = threadIdx.x % D;
    const int npass = (P + G - 1) / G;
    for (int pass = blockIdx.y; pass < npass; pass += gridDim.y) {
        const int p = pass * G + grp;
        const bool live = p < P;
        const int pc = live ? p : P - 1;
        const int i = pi[pc], j = pj[pc];
        const float *wrow = wtab[bil_wclamp(wmap[pc], g.NW)] + d * D;
        float w[D];
#pragma unroll
        for (int k = 0; k < D; ++k) w[k] = wrow[k];
        float *o = out + b0 * ldo + (int64_t)pc * D + d;
        for (int b = 0; b < nb; ++b) {
            const f32x4 *e4 = reinterpret_cast<const f32x4 *>(Et + b * FD + i * D);
            float u = 0.f;
#pragma unroll
            for (int k = 0; k < D; k += 4) {
                const f32x4 v = e4[k / 4];
                u += w[k] * v.x, u += w[k + 1] * v.y, u += w[k + 2] * v.z, u += w[k + 3] * v.w;
            }
            const float t = u * Et[b * FD + j * D + d];
            if (live) {
                o[b * ldo] = t;
                if (R > 0) o[b * ldo + (int64_t)P * D] = As[b * F + i] * As[b * F + j] * t;
            }
        }
    }
}

template <int D>
__device__ __forceinline__ void bil_load_w(const float *__restrict__ w, float *__restrict__ dst) {
    for (int e = threadIdx.x; e < D * D; e += BIL_T) dst[(e / D) * (D + 4) + (e % D)] = w[e];
}

// sample-major: dx (complete), the A scratch of the chunk, the workgroup's SENET partial
template <int D>
__global__ __launch_bounds__(BIL_T) void bil_bwd_rows_kernel(const float *__restrict__ dout, int64_t lddo,
                                                             const float *__restrict__ x, int64_t ldx,
                                                             const float *__restrict__ W1, const float *__restrict__ W2,
                                                             const float *const *__restrict__ wtab,
                                                             const int *__restrict__ wmap, float *__restrict__ dx,
                                                             int64_t lddx, int accumulate, float *__restrict__ ascr,
                                                             float *__restrict__ part, int first, int64_t B, BilGeom g) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    constexpr int TB = BIL_T / D, WS = D + 4;
    const int F = g.F, R = g.R, P = g.P, FD = F * D, r1 = R > 0 ? R : 1;
    float *Et = bil_lds, *dEt = Et + TB * FD, *Wl = dEt + TB * FD, *Zs = Wl + 2 * D * WS, *Hs = Zs + TB * F,
          *As = Hs + TB * r1, *dAs = As + TB * F, *dHs = dAs + TB * F, *dZs = dHs + TB * r1, *acc = dZs + TB * F;
    unsigned char *pi = reinterpret_cast<unsigned char *>(acc + 2 * R * F), *pj = pi + P;
    const int sb = threadIdx.x / D, d = threadIdx.x % D;
    const float inv = 1.f / (float)D;
    bil_pairs(F, pi, pj);
    for (int e = threadIdx.x; e < 2 * R * F; e += BIL_T) acc[e] = 0.f;
    const int64_t ntiles = (B + TB - 1) / TB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * TB;
        const int nb = B - b0 < TB ? (int)(B - b0) : TB;
        const bool live = sb < nb;
        const int64_t b = b0 + (live ? sb : 0);
        __syncthreads();  // the tile before is finished with everything below
        bil_stage(x, ldx, b0, nb, TB, FD, Et);
        for (int f = 0; f < F; ++f) dEt[sb * FD + f * D + d] = 0.f;
        for (int t = threadIdx.x; t < TB * F; t += BIL_T) dAs[t] = 0.f;
        bil_load_w<D>(wtab[bil_wclamp(wmap[0], g.NW)], Wl);
        __syncthreads();
        if (R > 0) {
            bil_senet(Et, TB, F, D, R, W1, W2, Zs, Hs, As);
            for (int t = threadIdx.x; t < nb * F; t += BIL_T) ascr[b0 * F + t] = As[t];
        }
        const float *gp_row = dout + b * lddo + d;
        for (int p = 0; p < P; ++p) {
            if (p + 1 < P) bil_load_w<D>(wtab[bil_wclamp(wmap[p + 1], g.NW)], Wl + ((p + 1) & 1) * D * WS);
            const float *W = Wl + (p & 1) * D * WS;
            const int i = pi[p], j = pj[p];
            const float gp = live ? gp_row[(int64_t)p * D] : 0.f;
            float gq = 0.f, s = 0.f, ai = 0.f, aj = 0.f;
            if (R > 0) {
                gq = live ? gp_row[(int64_t)(P + p) * D] : 0.f;
                ai = As[sb * F + i], aj = As[sb * F + j];
                s = ai * aj;
            }
            const float gg = gp + s * gq;
            const f32x4 *e4 = reinterpret_cast<const f32x4 *>(Et + sb * FD + i * D);
            const f32x4 *w4 = reinterpret_cast<const f32x4 *>(W + d * WS);
            float u = 0.f;
#pragma unroll
            for (int k = 0; k < D; k += 4) {
                const f32x4 v = e4[k / 4], w = w4[k / 4];
                u += w.x * v.x, u += w.y * v.y, u += w.z * v.z, u += w.w * v.w;
            }
            const float ej = Et[sb * FD + j * D + d];
            if (R > 0) {
                const float ds = rp_lane_sum_up<D>(gq * (u * ej));
                if (d == 0) dAs[sb * F + i] += ds * aj, dAs[sb * F + j] += ds * ai;
            }
            dEt[sb * FD + j * D + d] += gg * u;
            const float du = gg * ej;
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) a += W[k * WS + d] * __shfl(du, k, D);
            dEt[sb * FD + i * D + d] += a;
            __syncthreads();  // W_p is free, W_{p+1} is visible
        }
        if (R > 0) {
            for (int t = threadIdx.x; t < TB * F; t += BIL_T) dAs[t] = As[t] > 0.f ? dAs[t] : 0.f;  // through the second ReLU
            __syncthreads();
            for (int t = threadIdx.x; t < TB * R; t += BIL_T) {
                const int bb = t / R, r = t - bb * R;
                float sum = 0.f;
                for (int f = 0; f < F; ++f) sum += W2[f * R + r] * dAs[bb * F + f];
                dHs[t] = Hs[t] > 0.f ? sum : 0.f;  // through the first
            }
            __syncthreads();
            for (int e = threadIdx.x; e < 2 * R * F; e += BIL_T) {  // the rows behind nb hold exact zeros
                float sum = 0.f;
                if (e < R * F) {  // dW2 [F, R]
                    const int f = e / R, r = e - f * R;
                    for (int bb = 0; bb < TB; ++bb) sum += dAs[bb * F + f] * Hs[bb * R + r];
                } else {  // dW1 [R, F]
                    const int r = (e - R * F) / F, f = (e - R * F) - r * F;
                    for (int bb = 0; bb < TB; ++bb) sum += dHs[bb * R + r] * Zs[bb * F + f];
                }
                acc[e] += sum;
            }
            for (int t = threadIdx.x; t < TB * F; t += BIL_T) {
                const int bb = t / F, f = t - bb * F;
                float sum = 0.f;
                for (int r = 0; r < R; ++r) sum += W1[r * F + f] * dHs[bb * R + r];
                dZs[t] = sum * inv;
            }
            __syncthreads();
        }
        if (live) {
            float *o = dx + b * lddx + d;
            for (int f = 0; f < F; ++f) {
                float v = dEt[sb * FD + f * D + d];
                if (R > 0) v += dZs[sb * F + f];
                o[f * D] = accumulate ? o[f * D] + v : v;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * R * F; e += BIL_T) {
        float *slot = part + (size_t)blockIdx.x * 2 * R * F + e;
        *slot = first ? acc[e] : *slot + acc[e];
    }
}

// pair-major: workgroup (p, slice) -> its [D, D] partial of dW for pair p
template <int D>
__global__ __launch_bounds__(BIL_T) void bil_bwd_w_kernel(const float *__restrict__ dout, int64_t lddo,
                                                          const float *__restrict__ x, int64_t ldx,
                                                          const float *__restrict__ ascr, float *__restrict__ partw, int first,
                                                          int64_t B, int slen, BilGeom g) {
    __shared__ float dUs[BIL_WTILE * D], Eis[BIL_WTILE * D];
    constexpr int NE = (D * D + BIL_T - 1) / BIL_T;
    const int F = g.F, R = g.R, P = g.P, p = blockIdx.x;
    int i = 0, rem = p;
    while (rem >= F - 1 - i) rem -= F - 1 - i, ++i;
    const int j = i + 1 + rem;
    const int64_t bs = (int64_t)blockIdx.y * slen, be = bs + slen < B ? bs + slen : B;
    float acc[NE];
    int ek[NE], ed[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        const int e = threadIdx.x + m * BIL_T;
        acc[m] = 0.f, ek[m] = e % D, ed[m] = (e / D) % D;  // (e >= D D, D = 8 only: computed, never stored)
    }
    for (int64_t t0 = bs; t0 < be; t0 += BIL_WTILE) {
        const int n = be - t0 < BIL_WTILE ? (int)(be - t0) : BIL_WTILE;
        for (int idx = threadIdx.x; idx < BIL_WTILE * D; idx += BIL_T) {
            const int sb = idx / D, c = idx % D;
            float du = 0.f, ei = 0.f;
            if (sb < n) {
                const int64_t b = t0 + sb;
                const float *xr = x + b * ldx, *gr = dout + b * lddo + (int64_t)p * D + c;
                float gg = gr[0];
                if (R > 0) gg += ascr[b * F + i] * ascr[b * F + j] * gr[(int64_t)P * D];
                du = gg * xr[j * D + c], ei = xr[i * D + c];
            }
            dUs[idx] = du, Eis[idx] = ei;
        }
        __syncthreads();
        for (int sb = 0; sb < n; ++sb) {
#pragma unroll
            for (int m = 0; m < NE; ++m) acc[m] += dUs[sb * D + ed[m]] * Eis[sb * D + ek[m]];
        }
        __syncthreads();
    }
    float *slot = partw + ((size_t)blockIdx.y * P + p) * D * D;
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        const int e = threadIdx.x + m * BIL_T;
        if (e < D * D) slot[e] = first ? acc[m] : slot[e] + acc[m];
    }
}

// one thread per parameter element: dW [NW, D, D] (slices in order, then the pairs of the weight in order), dW2, dW1
__global__ __launch_bounds__(BIL_T) void bil_bwd_finish_kernel(const float *__restrict__ partw, int nsl,
                                                               const float *__restrict__ parts, int nblk,
                                                               const int *__restrict__ wmap, float *__restrict__ dW,
                                                               float *__restrict__ dW1, float *__restrict__ dW2, BilGeom g) {
    const int DD = g.D * g.D, RF = g.R * g.F;
    const int64_t idx = (int64_t)blockIdx.x * BIL_T + threadIdx.x;
    if (idx < (int64_t)g.NW * DD) {
        const int w = (int)(idx / DD), e = (int)(idx - (int64_t)w * DD);
        float s = 0.f;
        for (int p = 0; p < g.P; ++p) {
            if (bil_wclamp(wmap[p], g.NW) != w) continue;
            for (int sl = 0; sl < nsl; ++sl) s += partw[((size_t)sl * g.P + p) * DD + e];
        }
        dW[idx] = s;
        return;
    }
    const int64_t e = idx - (int64_t)g.NW * DD;
    if (e >= 2 * RF) return;
    float s = 0.f;
    for (int blk = 0; blk < nblk; ++blk) s += parts[(size_t)blk * 2 * RF + e];
    if (e < RF) dW2[e] = s;
    else dW1[e - RF] = s;
}

extern "C" int rp_bilinear_fits(int F, int D, int R, int type) {
    BilGeom g{};
    if (!bil_geom(F, D, R, type, &g)) return 0;
    return bil_fwd_lds_bytes(g, bil_fwd_tile(g)) <= BIL_FWD_LDS && bil_bwd_lds_bytes(g) <= BIL_BWD_LDS ? 1 : 0;
}

template <int D>
static void bil_fwd_launch(dim3 grid, size_t lds, hipStream_t s, const float *x, int64_t ldx, const float *W1, const float *W2,
                           const float *const *wtab, const int *wmap, float *out, int64_t ldo, int64_t B, int ND, int tb,
                           const BilGeom &g) {
    hipLaunchKernelGGL(bil_fwd_kernel<D>, grid, dim3(BIL_T), (unsigned)lds, s, x, ldx, W1, W2, wtab, wmap, out, ldo, B, ND, tb, g);
}

extern "C" int rp_bilinear_fwd(const float *x, int64_t ldx, const float *W1, const float *W2, const float *const *W,
                               const int *wmap, float *out, int64_t ldo, int F, int D, int R, int type, int n_dense, int64_t B,
                               rp_stream_t stream) {
    RP_REQUIRE(x && W && wmap && out && (R <= 0 || (W1 && W2)), "bilinear_fwd: null pointer");
    RP_REQUIRE(n_dense >= 0 && B >= 0, "bilinear_fwd: bad n_dense / B");
    BilGeom g{};
    if (!bil_geom(F, D, R, type, &g) || !rp_bilinear_fits(F, D, R, type))
        return rp_fail(RP_ERR_UNSUPPORTED, "bilinear_fwd: F=%d D=%d R=%d type=%d outside rp_bilinear_fits", F, D, R, type);
    const int64_t width = (int64_t)(R > 0 ? 2 : 1) * g.P * D + n_dense;
    RP_REQUIRE(ldx >= (int64_t)F * D + n_dense && ldo >= width, "bilinear_fwd: leading dimension too small");
    if (B == 0) return RP_OK;
    const int tb = bil_fwd_tile(g);
    const int64_t gx = rp_cdiv(B, tb);
    RP_REQUIRE(gx <= 0x7fffffff, "bilinear_fwd: B too large");
    const int npass = (int)rp_cdiv(g.P, BIL_T / D);
    int64_t gy = 1024 / gx;
    gy = gy < 1 ? 1 : (gy > npass ? npass : gy);
    const size_t lds = bil_fwd_lds_bytes(g, tb);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
        case 8: bil_fwd_launch<8>(grid, lds, s, x, ldx, W1, W2, W, wmap, out, ldo, B, n_dense, tb, g); break;
        case 16: bil_fwd_launch<16>(grid, lds, s, x, ldx, W1, W2, W, wmap, out, ldo, B, n_dense, tb, g); break;
        case 32: bil_fwd_launch<32>(grid, lds, s, x, ldx, W1, W2, W, wmap, out, ldo, B, n_dense, tb, g); break;
        default: bil_fwd_launch<64>(grid, lds, s, x, ldx, W1, W2, W, wmap, out, ldo, B, n_dense, tb, g); break;
    }
    RP_LAUNCH_CHECK("bilinear_fwd");
    return RP_OK;
}

// [BIL_SLICES][P][D D] pair partials | [BIL_BWD_BLOCKS][2 R F] SENET partials | [BIL_CHUNK][F] A scratch (R > 0), + alignment
static size_t bil_ws_floats(const BilGeom &g, size_t *parts_off, size_t *ascr_off) {
    size_t n = (size_t)BIL_SLICES * g.P * g.D * g.D;
    if (parts_off) *parts_off = n;
    n += (size_t)BIL_BWD_BLOCKS * 2 * g.R * g.F;
    if (ascr_off) *ascr_off = n;
    if (g.R > 0) n += (size_t)BIL_CHUNK * g.F;
    return n;
}

extern "C" int rp_bilinear_bwd_workspace_bytes(int F, int D, int R, int type, size_t *bytes) {
    RP_REQUIRE(bytes, "bilinear_bwd_workspace_bytes: null pointer");
    BilGeom g{};
    if (!bil_geom(F, D, R, type, &g) || !rp_bilinear_fits(F, D, R, type))
        return rp_fail(RP_ERR_UNSUPPORTED, "bilinear_bwd_workspace_bytes: F=%d D=%d R=%d type=%d outside rp_bilinear_fits", F, D,
                       R, type);
    *bytes = bil_ws_floats(g, nullptr, nullptr) * sizeof(float) + 256;
    return RP_OK;
}

template <int D>
static int bil_bwd_launch(hipStream_t s, const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *W1,
                          const float *W2, const float *const *wtab, const int *wmap, float *dx, int64_t lddx, int accumulate,
                          float *dW, float *dW1, float *dW2, int64_t B, float *partw, float *parts, float *ascr,
                          const BilGeom &g) {
    constexpr int TB = BIL_T / D;
    const size_t lds = bil_bwd_lds_bytes(g);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bil_bwd_rows_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    int nsl0 = 0, nblk0 = 0;
    for (int64_t c0 = 0; c0 < B; c0 += BIL_CHUNK) {
        const int64_t bc = B - c0 < BIL_CHUNK ? B - c0 : BIL_CHUNK;
        const int first = c0 == 0 ? 1 : 0;
        int64_t blocks = rp_cdiv(bc, TB);
        if (blocks > BIL_BWD_BLOCKS) blocks = BIL_BWD_BLOCKS;
        int64_t slen = rp_cdiv(bc, BIL_SLICES);
        if (slen < BIL_MIN_SLICE) slen = BIL_MIN_SLICE;
        const int nsl = (int)rp_cdiv(bc, slen);
        if (first) nsl0 = nsl, nblk0 = (int)blocks;  // (no later chunk is larger than the first)
        const float *dc = dout + c0 * lddo, *xc = x + c0 * ldx;
        hipLaunchKernelGGL(bil_bwd_rows_kernel<D>, dim3((unsigned)blocks), dim3(BIL_T), (unsigned)lds, s, dc, lddo, xc, ldx, W1, W2,
                           wtab, wmap, dx + c0 * lddx, lddx, accumulate, ascr, parts, first, bc, g);
        RP_LAUNCH_CHECK("bilinear_bwd (rows)");
        hipLaunchKernelGGL(bil_bwd_w_kernel<D>, dim3((unsigned)g.P, (unsigned)nsl), dim3(BIL_T), 0, s, dc, lddo, xc, ldx,
                           (const float *)ascr, partw, first, bc, (int)slen, g);
        RP_LAUNCH_CHECK("bilinear_bwd (wgrad)");
    }
    const int64_t n = (int64_t)g.NW * D * D + 2 * g.R * g.F;
    hipLaunchKernelGGL(bil_bwd_finish_kernel, dim3((unsigned)rp_cdiv(n, BIL_T)), dim3(BIL_T), 0, s, (const float *)partw, nsl0,
                       (const float *)parts, nblk0, wmap, dW, dW1, dW2, g);
    RP_LAUNCH_CHECK("bilinear_bwd (finish)");
    return RP_OK;
}

extern "C" int rp_bilinear_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *W1, const float *W2,
                               const float *const *W, const int *wmap, float *dx, int64_t lddx, int accumulate, float *dW,
                               float *dW1, float *dW2, int F, int D, int R, int type, int n_dense, int64_t B, void *workspace,
                               size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(dout && x && W && wmap && dx && dW && workspace && (R <= 0 || (W1 && W2 && dW1 && dW2)),
               "bilinear_bwd: null pointer");
    RP_REQUIRE(n_dense >= 0 && B >= 1, "bilinear_bwd: bad n_dense / B");
    BilGeom g{};
    if (!bil_geom(F, D, R, type, &g) || !rp_bilinear_fits(F, D, R, type))
        return rp_fail(RP_ERR_UNSUPPORTED, "bilinear_bwd: F=%d D=%d R=%d type=%d outside rp_bilinear_fits", F, D, R, type);
    const int64_t width = (int64_t)(R > 0 ? 2 : 1) * g.P * D + n_dense;
    RP_REQUIRE(ldx >= (int64_t)F * D && lddx >= (int64_t)F * D && lddo >= width, "bilinear_bwd: leading dimension too small");
    size_t parts_off = 0, ascr_off = 0;
    const size_t need = bil_ws_floats(g, &parts_off, &ascr_off) * sizeof(float) + 256;
    RP_REQUIRE(workspace_bytes >= need, "bilinear_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    float *ws = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    float *partw = ws, *parts = ws + parts_off, *ascr = ws + ascr_off;
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
        case 8: return bil_bwd_launch<8>(s, dout, lddo, x, ldx, W1, W2, W, wmap, dx, lddx, accumulate, dW, dW1, dW2, B, partw, parts, ascr, g);
        case 16: return bil_bwd_launch<16>(s, dout, lddo, x, ldx, W1, W2, W, wmap, dx, lddx, accumulate, dW, dW1, dW2, B, partw, parts, ascr, g);
        case 32: return bil_bwd_launch<32>(s, dout, lddo, x, ldx, W1, W2, W, wmap, dx, lddx, accumulate, dW, dW1, dW2, B, partw, parts, ascr, g);
        default: return bil_bwd_launch<64>(s, dout, lddo, x, ldx, W1, W2, W, wmap, dx, lddx, accumulate, dW, dW1, dW2, B, partw, parts, ascr, g);
    }
}
