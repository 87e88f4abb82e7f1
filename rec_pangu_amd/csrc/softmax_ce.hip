// Full-softmax cross entropy over the item vocabulary, forward and backward, gfx950 — the loss head of the sequence-recall
// family.  Reference: SequenceBaseModel.calculate_loss (rec_pangu/models/base_model.py:124-138):
//     scores = user_emb @ item_emb.weight.T        [B, V]
//     loss   = CrossEntropyLoss()(scores, target)  (mean over the batch)
// whose autograd keeps the logits, the softmax and their gradient: three [B, V] tensors.  Here no [B, V] tensor exists:
// score tiles of 32 x 32 live in the matrix core's accumulator registers, the forward leaves lse [B] and the loss, the
// backward recomputes each tile from U, E and lse.
//
// Notation: U [B, ldu >= D] fp32, E [V, D] fp32 contiguous, t [B] int64, s[b, v] = sum_d U[b, d] E[v, d].
//
// Products: v_mfma_f32_32x32x16_bf16 on split-bf16 operands (bfsplit.h), the product count from rp_matmul_products with the
// flops and bytes of the GEMM this launch stands for (logits included, as rp_linear_fwd counts its output): 1.5 D products
// per byte is below the ridge for every D the kernels take, so the automatic mode always runs the fp32-faithful 6 products;
// 3 and 1 are reached through rp_set_matmul_precision only (RP_MATMUL_FP32 runs 6 here: there is no f32-MFMA form).
// The recomputed probabilities are split into the same number of pieces as any other operand before the second product.
//
// Work split (a workgroup = 4 waves, every wave owns whole 32 x 32 tiles; fragments come straight from global memory, E and U
// tiles are re-read through L2):
//   forward   grid (ceil(B / 32), splits of V).  The workgroup's 32 rows of U stay in registers as B fragments; wave w takes the
//             tiles w, w + 4, ... of the split.  The tile is formed TRANSPOSED, S'[v, b] = E_tile . U_tile^T, so a lane holds 16
//             scores of ONE row b: the running maximum and sum (online softmax) are per-lane registers, the two lane halves
//             and the four waves are merged in a fixed order at the end, and one (m, l) pair per (row, split) goes to the
//             workspace.  sce_finish_kernel merges the pairs of a row (4 slices of the splits, each in ascending order, then
//             the slices in a fixed tree), adds the target's score as a plain fp32 dot product and leaves per-workgroup sums
//             of lse - s_t; st_mean_kernel adds those in a fixed order (the two-stage mean of lognet.hip / pair_loss.hip).
//   dU        same grid, tile orientation and product order, so the recomputed scores carry the forward's bits:
//             p' = exp(S' - lse) - [v == t_b] in registers.  (Seeding the accumulator with -lse instead rounds the sums at
//             the magnitude of lse a second, different time: at scores of +-470 the softmax of a peaked row then misses
//             exp(s_max - lse) = 1 / l by 1e-4 relative, measured, where the forward's own bits leave half an ulp of lse.)
//             dU^T[d, b] += E_tile^T . P' sums over the tile's ROW index v, so the accumulator registers are the next MFMA's
//             B operand as they are (no LDS, no lane movement).  The four waves' partial tiles are added in wave order, one
//             [B, D] slab per split goes to the workspace, st_slab_reduce_kernel adds the slabs in split order and scales by
//             g / B.
//   dE        grid ceil(V / 32): a workgroup owns 32 rows of E (in registers, B fragments) and walks ALL of B, wave w the row
//             tiles w, w + 4, ...; here the tile is S[b, v] = U_tile . E_tile^T (the same piece pairs in the same order) and
//             dE[v, d] += P'^T . U_tile sums over its row index b: the accumulator is the A operand.  Waves are added in wave
//             order; every row of dE has one writer.
// The one-hot is subtracted in the recomputed tile, so the target term needs no scatter and repeated targets no care.
// No floating-point atomics: all three results are bit-identical from run to run.
//
// D: any D >= 1 up to ST_MAX_D = 128; the contraction is zero-padded to a multiple of 32 (two k-steps of the MFMA; the dU / dE
// accumulators are 32 columns of D per tile).  D % 16 == 0 with 16-byte aligned rows loads fragments as two dwordx4.  Above
// 128 the pieces of the resident operand (3 x 4 registers per k-step) and the D / 32 output accumulators no longer fit beside
// the score tile without spilling: RP_ERR_ARG.
//
// The tile skeleton (constants, fragment loads, wave add, mean and slab-reduce kernels, split plan, dispatch) is score_tile.h,
// shared with contrast.hip; this file holds the softmax's own transform, (m, l) merge, finish kernel and workspace.
#include "score_tile.h"

#define SCE_SLICES 4       // lanes per row in the finishing merge
#define SCE_FROWS (ST_BLOCK / SCE_SLICES)

namespace {

// (m, l) <- the pair that stands for both sums; m = -inf marks "nothing yet"
__device__ __forceinline__ void sce_merge(float &m, float &l, float m2, float l2) {
    const float mm = fmaxf(m, m2);
    const float a = (m == -INFINITY) ? 0.f : expf(m - mm);
    const float b = (m2 == -INFINITY) ? 0.f : expf(m2 - mm);
    l = __fadd_rn(__fmul_rn(l, a), __fmul_rn(l2, b));
    m = mm;
}

__device__ __forceinline__ int64_t sce_target(const int64_t *__restrict__ t, int64_t b, int64_t V) {
    const int64_t v = t[b];
    return (v < 0 || v >= V) ? 0 : v;  // (flagged by the forward's finish; row 0 like the lookups)
}

template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void sce_fwd_kernel(const float *__restrict__ U, int64_t ldu,
                                                           const float *__restrict__ E, int64_t B, int64_t V, int D,
                                                           int64_t tps, int fastU, int fastE, float *__restrict__ ml) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float sm[ST_WAVES][32], sl[ST_WAVES][32];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * ST_TILE;
    const StTiles tr = st_split_tiles(V, tps);
    bf16x8 uf[KS][NP];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(U, ldu, b0 + r, b0 + r < B, 16 * ks + 8 * h, D, fastU), uf[ks]);
    float m = -INFINITY, l = 0.f;
    for (int64_t t = tr.t0 + w; t < tr.t1; t += ST_WAVES) {
        const int64_t v0 = t * ST_TILE;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 ef[NP];
            bf_split8<NP>(st_load8(E, D, v0 + r, v0 + r < V, 16 * ks + 8 * h, D, fastE), ef);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ef[BfProd<NPROD>::pa(pr)], uf[ks][BfProd<NPROD>::pb(pr)], acc, 0, 0, 0);
        }
        // acc[i] = s[b0 + r, v0 + rp_mfma32_row(i, h)]
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (v0 + rp_mfma32_row(i, h) >= V) acc[i] = -INFINITY;
            tm = fmaxf(tm, acc[i]);
        }
        if (tm > -INFINITY) {
            const float mn = fmaxf(m, tm);
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sum += expf(acc[i] - mn);  // (exp(-inf) = 0 for the rows beyond V)
            l = __fadd_rn(__fmul_rn(l, (m == -INFINITY) ? 0.f : expf(m - mn)), sum);
            m = mn;
        }
    }
    // the two lane halves hold different rows v of the same row b
    const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
    if (h == 0) {
        sce_merge(m, l, mo, lo);
        sm[w][r] = m;
        sl[w][r] = l;
    }
    __syncthreads();
    if (threadIdx.x < 32 && b0 + threadIdx.x < B) {
        float mm = sm[0][threadIdx.x], ll = sl[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < ST_WAVES; ++q) sce_merge(mm, ll, sm[q][threadIdx.x], sl[q][threadIdx.x]);
        float *o = ml + ((int64_t)blockIdx.y * B + b0 + threadIdx.x) * 2;
        o[0] = mm;
        o[1] = ll;
    }
}

// lse[b], the target's score and the workgroup's sum of lse - s_t.  SCE_SLICES lanes per row: slice q merges the splits
// q, q + SCE_SLICES, ... in ascending order, then the slices are merged by a fixed tree; the dot product the same way.
__global__ __launch_bounds__(ST_BLOCK) void sce_finish_kernel(const float *__restrict__ ml, int nsplit,
                                                              const float *__restrict__ U, int64_t ldu,
                                                              const float *__restrict__ E, const int64_t *__restrict__ tgt,
                                                              int64_t B, int64_t V, int D, float *__restrict__ lse,
                                                              float *__restrict__ partial, int32_t *__restrict__ err_flag) {
    __shared__ float sh[ST_WAVES];
    const int q = threadIdx.x % SCE_SLICES;
    const int64_t b = (int64_t)blockIdx.x * SCE_FROWS + threadIdx.x / SCE_SLICES;
    const bool valid = b < B;
    float m = -INFINITY, l = 0.f, dot = 0.f;
    if (valid) {
        for (int sp = q; sp < nsplit; sp += SCE_SLICES) {
            const float *p = ml + ((int64_t)sp * B + b) * 2;
            sce_merge(m, l, p[0], p[1]);
        }
        int64_t t = tgt[b];
        if (t < 0 || t >= V) {  // reference: IndexError from CrossEntropyLoss on the CPU
            if (q == 0) *err_flag = 1;
            t = 0;
        }
        const float *u = U + b * ldu, *e = E + t * D;
        for (int d = q; d < D; d += SCE_SLICES) dot = __builtin_fmaf(u[d], e[d], dot);
    }
#pragma unroll
    for (int o = 1; o < SCE_SLICES; o <<= 1) {
        const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
        // (both partners must form the same pair: the lower lane's operands first)
        if ((q & o) == 0) {
            sce_merge(m, l, mo, lo);
        } else {
            float m2 = mo, l2 = lo;
            sce_merge(m2, l2, m, l);
            m = m2;
            l = l2;
        }
        dot += __shfl_xor(dot, o, 64);
    }
    float term = 0.f;
    if (valid && q == 0) {
        const float v = m + logf(l);
        lse[b] = v;
        term = v - dot;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void sce_du_kernel(const float *__restrict__ U, int64_t ldu,
                                                          const float *__restrict__ E, const int64_t *__restrict__ tgt,
                                                          const float *__restrict__ lse, int64_t B, int64_t V, int D,
                                                          int64_t tps, int fastU, int fastE, float *__restrict__ dUp) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float red[(ST_WAVES - 1) * DT * 16 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * ST_TILE;
    const StTiles tr = st_split_tiles(V, tps);
    const bool bvalid = b0 + r < B;
    bf16x8 uf[KS][NP];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(U, ldu, b0 + r, bvalid, 16 * ks + 8 * h, D, fastU), uf[ks]);
    const float lse_b = bvalid ? lse[b0 + r] : 0.f;
    const int64_t tb = bvalid ? sce_target(tgt, b0 + r, V) : -1;
    f32x16 dacc[DT];  // dU^T[d = 32 dt + rp_mfma32_row(i, h), b = b0 + r]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dacc[dt][i] = 0.f;
    for (int64_t t = tr.t0 + w; t < tr.t1; t += ST_WAVES) {
        const int64_t v0 = t * ST_TILE;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 ef[NP];
            bf_split8<NP>(st_load8(E, D, v0 + r, v0 + r < V, 16 * ks + 8 * h, D, fastE), ef);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ef[BfProd<NPROD>::pa(pr)], uf[ks][BfProd<NPROD>::pb(pr)], acc, 0, 0, 0);
        }
        // acc[i] = s[b0 + r, v] at v = v0 + rp_mfma32_row(i, h), the forward's bits
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t v = v0 + rp_mfma32_row(i, h);
            acc[i] = (v < V && bvalid) ? expf(acc[i] - lse_b) - (v == tb ? 1.f : 0.f) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f32x8 pv;
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = acc[8 * s + j];
            bf16x8 pf[NP];
            bf_split8<NP>(pv, pf);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x8 af[NP];  // A[row d = 32 dt + r][k] = E[v0 + (row of k), d]
                bf_split8<NP>(st_load_rows(E, D, v0, V, s, h, 32 * dt + r, D), af);
#pragma unroll
                for (int pr = 0; pr < NPROD; ++pr)
                    dacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[BfProd<NPROD>::pa(pr)], pf[BfProd<NPROD>::pb(pr)], dacc[dt],
                                                                       0, 0, 0);
            }
        }
    }
    st_add_waves<DT>(dacc, red, w, lane);
    if (w == 0 && bvalid) {
        float *o = dUp + ((int64_t)blockIdx.y * B + b0 + r) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int d = 32 * dt + rp_mfma32_row(i, h);
                if (d < D) o[d] = dacc[dt][i];
            }
    }
}

template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void sce_de_kernel(const float *__restrict__ U, int64_t ldu,
                                                          const float *__restrict__ E, const int64_t *__restrict__ tgt,
                                                          const float *__restrict__ lse, const float *__restrict__ gloss,
                                                          float inv_b, int64_t B, int64_t V, int D, int fastU, int fastE,
                                                          float *__restrict__ dE) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float red[(ST_WAVES - 1) * DT * 16 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t v0 = (int64_t)blockIdx.x * ST_TILE;
    const int64_t btiles = (B + 31) / 32;
    bf16x8 ef[KS][NP];  // B[k][col r] = E[v0 + r, k]
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(E, D, v0 + r, v0 + r < V, 16 * ks + 8 * h, D, fastE), ef[ks]);
    f32x16 zacc[DT];  // dE[v = v0 + rp_mfma32_row(i, h), d = 32 dt + r]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) zacc[dt][i] = 0.f;
    for (int64_t bt = w; bt < btiles; bt += ST_WAVES) {
        const int64_t b0 = bt * 32;
        f32x16 acc;
        float lse_r[16], hit[16];  // lse[b] and [v0 + r == t_b] of register row b; hit = -1 marks a row beyond B
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t b = b0 + rp_mfma32_row(i, h);
            const bool ok = b < B;
            acc[i] = 0.f;
            lse_r[i] = ok ? lse[b] : 0.f;
            hit[i] = ok ? ((sce_target(tgt, b, V) == v0 + r) ? 1.f : 0.f) : -1.f;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 uf[NP];
            bf_split8<NP>(st_load8(U, ldu, b0 + r, b0 + r < B, 16 * ks + 8 * h, D, fastU), uf);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                // (the forward pairs piece pa of E with piece pb of U: the same pairs in the same order here)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uf[BfProd<NPROD>::pb(pr)], ef[ks][BfProd<NPROD>::pa(pr)], acc, 0, 0, 0);
        }
        // acc[i] = s[b, v0 + r] at b = b0 + rp_mfma32_row(i, h)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = (hit[i] >= 0.f) ? expf(acc[i] - lse_r[i]) - hit[i] : 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f32x8 pv;
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = acc[8 * s + j];
            bf16x8 pf[NP];  // A[row v = r][k] = P'[b0 + (row of k), v0 + r]
            bf_split8<NP>(pv, pf);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x8 bf[NP];  // B[k][col d = 32 dt + r] = U[b0 + (row of k), d]
                bf_split8<NP>(st_load_rows(U, ldu, b0, B, s, h, 32 * dt + r, D), bf);
#pragma unroll
                for (int pr = 0; pr < NPROD; ++pr)
                    zacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[BfProd<NPROD>::pa(pr)], bf[BfProd<NPROD>::pb(pr)], zacc[dt],
                                                                       0, 0, 0);
            }
        }
    }
    st_add_waves<DT>(zacc, red, w, lane);
    if (w == 0) {
        const float scale = gloss[0] * inv_b;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = 32 * dt + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t v = v0 + rp_mfma32_row(i, h);
                if (v < V && d < D) dE[v * D + d] = zacc[dt][i] * scale;
            }
        }
    }
}

struct SceWs {
    float *ml, *partial, *dup;
    size_t bytes;
};

SceWs sce_workspace(void *base, int64_t B, int D, const StPlan &g) {
    SceWs w;
    const size_t n_ml = (size_t)2 * g.nsplit * B, n_part = (size_t)rp_cdiv(B, SCE_FROWS);
    const size_t n_dup = (size_t)g.nsplit * B * D;
    w.ml = reinterpret_cast<float *>(base);
    w.partial = w.ml + n_ml;
    w.dup = w.partial + ((n_part + 3) & ~(size_t)3);
    w.bytes = (n_ml + ((n_part + 3) & ~(size_t)3) + n_dup) * sizeof(float);
    return w;
}

}  // namespace

extern "C" int rp_softmax_ce_geometry(int *tb, int *tv, int *max_d, int *slices) {
    RP_REQUIRE(tb && tv && max_d && slices, "softmax_ce_geometry: null pointer");
    *tb = ST_TILE;
    *tv = ST_TILE;
    *max_d = ST_MAX_D;
    *slices = SCE_SLICES;
    return RP_OK;
}

extern "C" int rp_softmax_ce_splits(int64_t B, int64_t V, int *nsplit, int64_t *tiles_per_split) {
    RP_REQUIRE(nsplit && tiles_per_split, "softmax_ce_splits: null pointer");
    RP_REQUIRE(B >= 1 && V >= 1, "softmax_ce_splits: B and V must be positive");
    const StPlan g = st_plan(B, V);
    *nsplit = g.nsplit;
    *tiles_per_split = g.tps;
    return RP_OK;
}

extern "C" int rp_softmax_ce_workspace_bytes(int64_t B, int64_t V, int D, size_t *bytes) {
    RP_REQUIRE(bytes, "softmax_ce_workspace_bytes: null pointer");
    RP_REQUIRE(B >= 1 && V >= 1 && D >= 1, "softmax_ce_workspace_bytes: B, V and D must be positive");
    *bytes = sce_workspace(nullptr, B, D, st_plan(B, V)).bytes;
    return RP_OK;
}

extern "C" int rp_softmax_ce_fwd(const float *U, int64_t ldu, const float *E, const int64_t *target, int64_t B, int64_t V, int D,
                                 float *lse, float *loss, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                                 rp_stream_t stream) {
    RP_REQUIRE(U && E && target && lse && loss && err_flag && workspace, "softmax_ce_fwd: null pointer");
    RP_REQUIRE(B >= 1 && V >= 1 && D >= 1 && ldu >= D, "softmax_ce_fwd: bad B / V / D / ldu");
    RP_REQUIRE(D <= ST_MAX_D, "softmax_ce_fwd: D=%d above the %d the register budget takes", D, ST_MAX_D);
    const StPlan g = st_plan(B, V);
    const SceWs ws = sce_workspace(workspace, B, D, g);
    RP_REQUIRE(workspace_bytes >= ws.bytes && rp_aligned16(workspace), "softmax_ce_fwd: workspace too small or misaligned");
    const int dt = (D + 31) / 32, nprod = st_products(B, V, D);
    const int fu = st_fast(U, ldu, D), fe = st_fast(E, D, D);
    hipStream_t s = (hipStream_t)stream;
#define CALL(DT_, NP_)                                                                                                      \
    hipLaunchKernelGGL((sce_fwd_kernel<DT_, NP_>), dim3((unsigned)g.row_tiles, (unsigned)g.nsplit), dim3(ST_BLOCK), 0, s, U,  \
                       ldu, E, B, V, D, g.tps, fu, fe, ws.ml)
    ST_DISPATCH(dt, nprod, CALL);
#undef CALL
    RP_LAUNCH_CHECK("softmax_ce_fwd");
    const int64_t nb = rp_cdiv(B, SCE_FROWS);
    hipLaunchKernelGGL(sce_finish_kernel, dim3((unsigned)nb), dim3(ST_BLOCK), 0, s, ws.ml, g.nsplit, U, ldu, E, target, B, V, D,
                       lse, ws.partial, err_flag);
    RP_LAUNCH_CHECK("softmax_ce_finish");
    hipLaunchKernelGGL(st_mean_kernel, dim3(1), dim3(ST_BLOCK), 0, s, ws.partial, nb, 1.f / (float)B, loss);
    RP_LAUNCH_CHECK("softmax_ce_mean");
    return RP_OK;
}

extern "C" int rp_softmax_ce_bwd(const float *U, int64_t ldu, const float *E, const int64_t *target, const float *lse,
                                 const float *gloss, int64_t B, int64_t V, int D, float *dU, int64_t lddu, float *dE,
                                 void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(U && E && target && lse && gloss && workspace, "softmax_ce_bwd: null pointer");
    RP_REQUIRE(dU || dE, "softmax_ce_bwd: neither gradient asked for");
    RP_REQUIRE(B >= 1 && V >= 1 && D >= 1 && ldu >= D && (!dU || lddu >= D), "softmax_ce_bwd: bad B / V / D / ldu / lddu");
    RP_REQUIRE(D <= ST_MAX_D, "softmax_ce_bwd: D=%d above the %d the register budget takes", D, ST_MAX_D);
    const StPlan g = st_plan(B, V);
    const SceWs ws = sce_workspace(workspace, B, D, g);
    RP_REQUIRE(workspace_bytes >= ws.bytes && rp_aligned16(workspace), "softmax_ce_bwd: workspace too small or misaligned");
    const int dt = (D + 31) / 32, nprod = st_products(B, V, D);
    const int fu = st_fast(U, ldu, D), fe = st_fast(E, D, D);
    const float inv_b = 1.f / (float)B;
    hipStream_t s = (hipStream_t)stream;
    if (dU) {
#define CALL(DT_, NP_)                                                                                                     \
    hipLaunchKernelGGL((sce_du_kernel<DT_, NP_>), dim3((unsigned)g.row_tiles, (unsigned)g.nsplit), dim3(ST_BLOCK), 0, s, U,  \
                       ldu, E, target, lse, B, V, D, g.tps, fu, fe, ws.dup)
        ST_DISPATCH(dt, nprod, CALL);
#undef CALL
        RP_LAUNCH_CHECK("softmax_ce_du");
        int64_t nb = rp_cdiv(B * D, ST_BLOCK);
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(st_slab_reduce_kernel, dim3((unsigned)nb), dim3(ST_BLOCK), 0, s, ws.dup, g.nsplit, B, D, nullptr,
                           gloss, inv_b, dU, lddu);
        RP_LAUNCH_CHECK("softmax_ce_du_reduce");
    }
    if (dE) {
#define CALL(DT_, NP_)                                                                                                    \
    hipLaunchKernelGGL((sce_de_kernel<DT_, NP_>), dim3((unsigned)g.tiles), dim3(ST_BLOCK), 0, s, U, ldu, E, target, lse, gloss,  \
                       inv_b, B, V, D, fu, fe, dE)
        ST_DISPATCH(dt, nprod, CALL);
#undef CALL
        RP_LAUNCH_CHECK("softmax_ce_de");
    }
    return RP_OK;
}
