// AOANet's generalized interaction layer (ranking/aoanet.py:97-115) without its outer product, fp32, gfx950.
//
// rp_gin_*   reference: out = ((W * sum_n alpha[n, o] (X0[n % F] (x) Bi[n / F])) . h), n = p F + f — the reference builds the
//            [B, P F, D, D] outer product first (2.8 MB per sample at F = P = 26, D = 32).  Factorised:
//                M[o,h,d] = W[o,h,d] h[o,d]
//                T[b,o,p,h] = sum_d M[o,h,d] Bi[b,p,d]        U[b,o,p,h] = sum_f alpha[p F + f, o] X0[b,f,h]
//                out[b,o,h] = sum_p T U
//            T and U live one (o, p) at a time in a register of the thread that owns (sample, h); nothing of size
//            B O P D reaches global memory, forward or backward — the backward rebuilds T and U from X0, Bi and the parameters.
//
// One workgroup of 256 threads owns a tile of S = 256 / D samples (fewer when the tile would not fit in LDS): thread
// t = (s, h).  The tile's X0 rows sit in LDS with a field stride of D + 1 floats — the (s, h) threads read down a column
// (consecutive h: conflict-free), the dalpha phase reads across fields (stride D + 1, odd: conflict-free) — and a sample
// stride congruent to D mod 32: for D < 32 the several samples of one 32-lane group then land on disjoint banks (for D = 32
// and 64 a 32-lane group lies inside one sample and any stride is conflict-free).  The Bi rows are contiguous
// (p D + d: ds_read_b128, the lanes of a sample broadcast) with a sample stride congruent to D mod 64.  M's row h (and,
// in the backward, its column) is held in 2 D registers per o; alpha is read with wave-uniform addresses.
//
// Backward, per tile, per o, per chunk of GIN_PC values of p:
//   phase A  thread (s, h): T, U again; dU = g T, dT = g U into LDS ([pp][s D + h]); dX0[s,f,h] += alpha dU in an LDS
//            accumulator only its owner touches.
//   phase B  dBi[s,p,d] += sum_h M[o,h,d] dT[s,p,h]           thread (s, d), LDS accumulator of its own
//            dalpha[pF+f, o] = sum_{s,h} X0[s,f,h] dU[s,p,h]   thread per (pp, f) pair
//            dM[o,h,d] += sum_{s,pp} dT[s,pp,h] Bi[s,p,d]      thread per (h, d)
//            the last two into the workgroup's OWN partial in the workspace (written by the first tile, added to by the
//            later ones of its grid-stride walk), summed over the workgroups in a fixed order by the finishing launch, which
//            also forms dW = dM h and dh = sum_h dM W.  No floating-point atomics: bit-identical from run to run; the
//            workspace is GIN_BWD_BLOCKS partials whatever the batch.
#include "common.h"

#define GIN_THREADS 256
#define GIN_PC 8              // values of p per backward chunk
#define GIN_KP 257            // row stride of the dU / dT exchange tiles (odd; k = s D + h < 256)
#define GIN_FWD_BLOCKS 512    // grid caps (grid-stride over the sample tiles beyond): two resident workgroups per CU
#define GIN_BWD_BLOCKS 256    // = partials in the workspace
#define GIN_LDS_FLOATS 36864  // 144 KiB of the CU's 160
#define GIN_MAXF 64
#define GIN_MAXO 16

struct GinGeom {
    int S, RS, BS;  // samples per tile, sample strides of the X0 and the Bi tile (floats)
    int lds_floats;
};

static inline int gin_pad_to(int n, int r, int mod) { return n + (((r - n) % mod) + mod) % mod; }  // >= n, = r (mod)

static bool gin_supported_d(int D) { return D == 8 || D == 16 || D == 20 || D == 32 || D == 64; }

static bool gin_geom(int F, int P, int O, int D, bool bwd, GinGeom *g) {
    if (!gin_supported_d(D) || F < 1 || P < 1 || O < 1 || F > GIN_MAXF || P > GIN_MAXF || O > GIN_MAXO) return false;
    g->RS = gin_pad_to(F * (D + 1), D % 32, 32);
    g->BS = gin_pad_to(P * D, D % 64, 64);
    const int per = (bwd ? 2 : 1) * (g->RS + g->BS), fixed = (bwd ? 2 * GIN_PC * GIN_KP : 0) + 16;
    int S = (GIN_LDS_FLOATS - fixed) / per;
    if (S > GIN_THREADS / D) S = GIN_THREADS / D;
    if (S < 1) return false;
    g->S = S;
    g->lds_floats = (bwd ? 2 : 1) * (rp_round_up(S * g->RS, 4) + rp_round_up(S * g->BS, 4)) +
                    (bwd ? 2 * rp_round_up(GIN_PC * GIN_KP, 4) : 0);
    return true;
}

// the tile's rows of a [B, ld] operand (n = fields * D floats each) into LDS: element (s, f, h) at s * SS + f * FS + h;
// samples beyond B as zeros
template <int D>
__device__ __forceinline__ void gin_stage(const float *__restrict__ src, int64_t ld, int64_t b0, int64_t B, int S, int nf,
                                          int SS, int FS, float *__restrict__ dst) {
    const int n = nf * D;
    for (int i = threadIdx.x; i < S * n; i += GIN_THREADS) {
        const int s = i / n, c = i - s * n, f = c / D, h = c - f * D;
        dst[s * SS + f * FS + h] = (b0 + s < B) ? src[(b0 + s) * ld + c] : 0.f;
    }
}

template <int D>
__device__ __forceinline__ float gin_dot_row(const float (&m)[D], const float *__restrict__ brow) {
    const f32x4 *bq = reinterpret_cast<const f32x4 *>(brow);
    float T = 0.f;
#pragma unroll
    for (int q = 0; q < D / 4; ++q) {
        const f32x4 v = bq[q];
        T += m[4 * q] * v.x + m[4 * q + 1] * v.y + m[4 * q + 2] * v.z + m[4 * q + 3] * v.w;
    }
    return T;
}

template <int D>
__global__ __launch_bounds__(GIN_THREADS) void gin_fwd_kernel(const float *__restrict__ x0, int64_t ldx0,
                                                              const float *__restrict__ bi, int64_t ldbi,
                                                              const float *__restrict__ W,
                                                              const float *__restrict__ alpha,
                                                              const float *__restrict__ hv, float *__restrict__ out,
                                                              int64_t ldo, int F, int P, int O, int64_t B, int S, int RS,
                                                              int BS) {
    extern __shared__ __attribute__((aligned(16))) float gin_lds[];
    constexpr int DP = D + 1;
    float *xs = gin_lds, *bs = xs + ((S * RS + 3) & ~3);
    const int t = threadIdx.x, s = t / D, h = t - s * D;
    const bool act = s < S;
    const int64_t ntiles = (B + S - 1) / S;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        gin_stage<D>(x0, ldx0, b0, B, S, F, RS, DP, xs);
        gin_stage<D>(bi, ldbi, b0, B, S, P, BS, D, bs);
        __syncthreads();
        if (act && b0 + s < B) {
            const float *xcol = xs + s * RS + h, *brow = bs + s * BS;
            float *orow = out + (b0 + s) * ldo + h;
            for (int o = 0; o < O; ++o) {
                float m[D];
                const float *wr = W + ((int64_t)o * D + h) * D, *hr = hv + o * D;
#pragma unroll
                for (int d = 0; d < D; ++d) m[d] = wr[d] * hr[d];
                float acc = 0.f;
                for (int p = 0; p < P; ++p) {
                    const float T = gin_dot_row<D>(m, brow + p * D);
                    const float *ap = alpha + (int64_t)p * F * O + o;
                    float U = 0.f;
                    for (int f = 0; f < F; ++f) U += ap[f * O] * xcol[f * DP];
                    acc += T * U;
                }
                orow[o * D] = acc;
            }
        }
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(GIN_THREADS) void gin_bwd_kernel(const float *__restrict__ dout, int64_t lddo,
                                                              const float *__restrict__ x0, int64_t ldx0,
                                                              const float *__restrict__ bi, int64_t ldbi,
                                                              const float *__restrict__ W,
                                                              const float *__restrict__ alpha,
                                                              const float *__restrict__ hv, float *__restrict__ dx0,
                                                              int64_t lddx0, int accumulate, float *__restrict__ dbi,
                                                              int64_t lddbi, float *__restrict__ part, int F, int P,
                                                              int O, int64_t B, int S, int RS, int BS) {
    extern __shared__ __attribute__((aligned(16))) float gin_lds[];
    constexpr int DP = D + 1;
    const int nx = (S * RS + 3) & ~3, nb = (S * BS + 3) & ~3, ne = (GIN_PC * GIN_KP + 3) & ~3;
    float *xs = gin_lds, *bs = xs + nx, *dxs = bs + nb, *dbs = dxs + nx, *du = dbs + nb, *dt = du + ne;
    const int t = threadIdx.x, s = t / D, h = t - s * D;
    const bool act = s < S;
    const int nA = P * F * O;
    float *pA = part + (int64_t)blockIdx.x * (nA + O * D * D), *pM = pA + nA;
    const int64_t ntiles = (B + S - 1) / S;
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        gin_stage<D>(x0, ldx0, b0, B, S, F, RS, DP, xs);
        gin_stage<D>(bi, ldbi, b0, B, S, P, BS, D, bs);
        for (int i = t; i < nx + nb; i += GIN_THREADS) dxs[i] = 0.f;  // (dxs and dbs are adjacent)
        __syncthreads();
        const bool live = act && b0 + s < B;
        const float *xcol = xs + s * RS + h, *brow = bs + s * BS;
        float *dxcol = dxs + s * RS + h;
        for (int o = 0; o < O; ++o) {
            float m[D], mt[D];  // row h and column h of M[o]
            if (act) {
                const float *wo = W + (int64_t)o * D * D, *hr = hv + o * D;
                const float hh = hr[h];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    m[d] = wo[h * D + d] * hr[d];
                    mt[d] = wo[d * D + h] * hh;
                }
            }
            const float g = live ? dout[(b0 + s) * lddo + o * D + h] : 0.f;
            for (int pc = 0; pc < P; pc += GIN_PC) {
                const int np = P - pc < GIN_PC ? P - pc : GIN_PC;
                if (act) {
                    for (int pp = 0; pp < np; ++pp) {
                        const int p = pc + pp;
                        const float T = gin_dot_row<D>(m, brow + p * D);
                        const float dU = g * T;
                        const float *ap = alpha + (int64_t)p * F * O + o;
                        float U = 0.f;
                        for (int f = 0; f < F; ++f) {
                            const float a = ap[f * O];
                            U += a * xcol[f * DP];
                            dxcol[f * DP] += a * dU;
                        }
                        du[pp * GIN_KP + t] = dU;
                        dt[pp * GIN_KP + t] = g * U;
                    }
                }
                __syncthreads();
                if (act) {  // dBi[s, p, d = h] += sum_j M[o, j, h] dT[s, p, j]
                    for (int pp = 0; pp < np; ++pp) {
                        const float *dr = dt + pp * GIN_KP + s * D;
                        float a = 0.f;
#pragma unroll
                        for (int j = 0; j < D; ++j) a += mt[j] * dr[j];
                        dbs[s * BS + (pc + pp) * D + h] += a;
                    }
                }
                for (int j = t; j < np * F; j += GIN_THREADS) {  // dalpha[(pc + pp) F + f, o] over the tile
                    const int pp = j / F, f = j - pp * F;
                    const float *ur = du + pp * GIN_KP, *xf = xs + f * DP;
                    float a = 0.f;
                    for (int ss = 0; ss < S; ++ss)
#pragma unroll 4
                        for (int hh = 0; hh < D; ++hh) a += xf[ss * RS + hh] * ur[ss * D + hh];
                    float *dst = pA + ((int64_t)(pc + pp) * F + f) * O + o;
                    *dst = first ? a : *dst + a;
                }
                for (int e = t; e < D * D; e += GIN_THREADS) {  // dM[o, hh, d] over the tile and this chunk's p
                    const int hh = e / D, d = e - hh * D;
                    float a = 0.f;
                    for (int pp = 0; pp < np; ++pp) {
                        const float *tr = dt + pp * GIN_KP + hh, *br = bs + (pc + pp) * D + d;
                        for (int ss = 0; ss < S; ++ss) a += tr[ss * D] * br[ss * BS];
                    }
                    float *dst = pM + (int64_t)o * D * D + e;
                    *dst = (first && pc == 0) ? a : *dst + a;
                }
                __syncthreads();
            }
        }
        // the tile's data gradients leave LDS once
        const int nfd = F * D, npd = P * D;
        for (int i = t; i < S * nfd; i += GIN_THREADS) {
            const int ss = i / nfd, c = i - ss * nfd, f = c / D, hh = c - f * D;
            if (b0 + ss < B) {
                float v = dxs[ss * RS + f * DP + hh];
                if (dbi == nullptr) v += dbs[ss * BS + c];  // bi IS x0 (P == F): both roles' gradients in one row
                float *dst = dx0 + (b0 + ss) * lddx0 + c;
                *dst = accumulate ? *dst + v : v;
            }
        }
        if (dbi != nullptr) {
            for (int i = t; i < S * npd; i += GIN_THREADS) {
                const int ss = i / npd, c = i - ss * npd;
                if (b0 + ss < B) dbi[(b0 + ss) * lddbi + c] = dbs[ss * BS + c];
            }
        }
        first = false;
        __syncthreads();
    }
}

// blocks [0, ablocks): dalpha, one element per thread.  The others: (o, 16 columns d) x 16 slices of h — a thread sums its
// elements' partials over the workgroups in order, writes dW = dM h, and the slices' shares of dh = sum_h dM W combine in order
__global__ __launch_bounds__(256) void gin_bwd_finish_kernel(const float *__restrict__ part, int nblk, int nA, int O, int D,
                                                             const float *__restrict__ W,
                                                             const float *__restrict__ hv, float *__restrict__ dalpha,
                                                             float *__restrict__ dW, float *__restrict__ dh,
                                                             int ablocks) {
    __shared__ float red[256];
    const int64_t stride = (int64_t)nA + (int64_t)O * D * D;
    if ((int)blockIdx.x < ablocks) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < nA) {
            float a = 0.f;
            for (int b = 0; b < nblk; ++b) a += part[b * stride + i];
            dalpha[i] = a;
        }
        return;
    }
    const int bid = blockIdx.x - ablocks, ncg = (D + 15) / 16;
    const int o = bid / ncg, c = threadIdx.x & 15, sl = threadIdx.x >> 4, d = (bid - o * ncg) * 16 + c;
    float acc = 0.f;
    if (d < D) {
        const float hd = hv[o * D + d];
        for (int hh = sl; hh < D; hh += 16) {
            const int e = (o * D + hh) * D + d;
            float a = 0.f;
            for (int b = 0; b < nblk; ++b) a += part[b * stride + nA + e];
            dW[e] = a * hd;
            acc += a * W[e];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (sl == 0 && d < D) {
        for (int k = 1; k < 16; ++k) acc += red[k * 16 + c];
        dh[o * D + d] = acc;
    }
}

#define GIN_DISPATCH(D, CALL)     \
    switch (D) {                  \
        case 8: CALL(8); break;   \
        case 16: CALL(16); break; \
        case 20: CALL(20); break; \
        case 32: CALL(32); break; \
        default: CALL(64); break; \
    }

extern "C" int rp_gin_fits(int F, int P, int O, int D) {
    GinGeom g;
    return (gin_geom(F, P, O, D, false, &g) && gin_geom(F, P, O, D, true, &g)) ? 1 : 0;
}

extern "C" int rp_gin_fwd(const float *x0, int64_t ldx0, const float *bi, int64_t ldbi, const float *W, const float *alpha,
                          const float *h, float *out, int64_t ldo, int F, int P, int O, int D, int64_t B,
                          rp_stream_t stream) {
    RP_REQUIRE(x0 && bi && W && alpha && h && out, "gin_fwd: null pointer");
    RP_REQUIRE(F >= 1 && P >= 1 && O >= 1 && D >= 1 && B >= 0, "gin_fwd: bad F / P / O / D / B");
    RP_REQUIRE(ldx0 >= (int64_t)F * D && ldbi >= (int64_t)P * D && ldo >= (int64_t)O * D,
               "gin_fwd: leading dimension too small");
    GinGeom g;
    if (!gin_geom(F, P, O, D, false, &g))
        return rp_fail(RP_ERR_UNSUPPORTED, "gin_fwd: F=%d P=%d O=%d D=%d outside rp_gin_fits", F, P, O, D);
    if (B == 0) return RP_OK;
    int64_t blocks = rp_cdiv(B, g.S);
    if (blocks > GIN_FWD_BLOCKS) blocks = GIN_FWD_BLOCKS;
    const size_t lds = (size_t)g.lds_floats * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define CALL(DD)                                                                                                         \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gin_fwd_kernel<DD>),                                        \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                     \
    hipLaunchKernelGGL((gin_fwd_kernel<DD>), dim3((unsigned)blocks), dim3(GIN_THREADS), (unsigned)lds, s, x0, ldx0, bi, \
                       ldbi, W, alpha, h, out, ldo, F, P, O, B, g.S, g.RS, g.BS)
    GIN_DISPATCH(D, CALL)
#undef CALL
    RP_LAUNCH_CHECK("gin_fwd");
    return RP_OK;
}

extern "C" int rp_gin_bwd_workspace_bytes(int F, int P, int O, int D, size_t *bytes) {
    RP_REQUIRE(bytes && F >= 1 && P >= 1 && O >= 1 && D >= 1, "gin_bwd_workspace_bytes: bad argument");
    *bytes = (size_t)GIN_BWD_BLOCKS * ((size_t)P * F * O + (size_t)O * D * D) * sizeof(float) + 256;
    return RP_OK;
}

extern "C" int rp_gin_bwd(const float *dout, int64_t lddo, const float *x0, int64_t ldx0, const float *bi, int64_t ldbi,
                          const float *W, const float *alpha, const float *h, float *dx0, int64_t lddx0, int accumulate,
                          float *dbi, int64_t lddbi, float *dW, float *dalpha, float *dh, int F, int P, int O, int D,
                          int64_t B, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(dout && x0 && bi && W && alpha && h && dx0 && dW && dalpha && dh && workspace, "gin_bwd: null pointer");
    RP_REQUIRE(F >= 1 && P >= 1 && O >= 1 && D >= 1 && B >= 1, "gin_bwd: bad F / P / O / D / B");
    RP_REQUIRE(ldx0 >= (int64_t)F * D && ldbi >= (int64_t)P * D && lddo >= (int64_t)O * D && lddx0 >= (int64_t)F * D,
               "gin_bwd: leading dimension too small");
    RP_REQUIRE(dbi ? lddbi >= (int64_t)P * D : (bi == x0 && ldbi == ldx0 && P == F),
               "gin_bwd: dbi may be NULL only where bi is x0 itself (its gradient then joins dx0)");
    GinGeom g;
    if (!gin_geom(F, P, O, D, true, &g))
        return rp_fail(RP_ERR_UNSUPPORTED, "gin_bwd: F=%d P=%d O=%d D=%d outside rp_gin_fits", F, P, O, D);
    size_t need = 0;
    rp_gin_bwd_workspace_bytes(F, P, O, D, &need);
    RP_REQUIRE(workspace_bytes >= need, "gin_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    float *part = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int64_t blocks = rp_cdiv(B, g.S);
    if (blocks > GIN_BWD_BLOCKS) blocks = GIN_BWD_BLOCKS;
    const size_t lds = (size_t)g.lds_floats * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define CALL(DD)                                                                                                          \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gin_bwd_kernel<DD>),                                         \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                      \
    hipLaunchKernelGGL((gin_bwd_kernel<DD>), dim3((unsigned)blocks), dim3(GIN_THREADS), (unsigned)lds, s, dout, lddo, x0, \
                       ldx0, bi, ldbi, W, alpha, h, dx0, lddx0, accumulate, dbi, lddbi, part, F, P, O, B, g.S, g.RS, g.BS)
    GIN_DISPATCH(D, CALL)
#undef CALL
    RP_LAUNCH_CHECK("gin_bwd");
    const int nA = P * F * O, ablocks = (int)rp_cdiv(nA, 256);
    hipLaunchKernelGGL(gin_bwd_finish_kernel, dim3((unsigned)(ablocks + O * ((D + 15) / 16))), dim3(256), 0, s, part,
                       (int)blocks, nA, O, D, W, h, dalpha, dW, dh, ablocks);
    RP_LAUNCH_CHECK("gin_bwd (finish)");
    return RP_OK;
}
