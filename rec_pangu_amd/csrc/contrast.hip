// In-batch contrastive loss (a softmax over the similarities between the rows of one batch, positives by equal label),
// forward and backward, gfx950 — the loss of CLRec (models/sequence/clrec.py:65-102 of the reference) and of ContraRec
// (contrarec.py:93-144).  The reference materialises the [n, m] matrix about seven times (dot, logits, mask, logits_mask,
// exp_logits, log_prob, mask * log_prob) and autograd keeps most of them.  Here no [n, m] tensor exists: this is the sibling
// of softmax_ce.hip on the one skeleton of score_tile.h — the same 32 x 32 score tiles in the matrix core's accumulators, the
// same orientations, the same rule that the recomputed tile carries the forward's bits.
//
// Notation: a [n, lda >= D], b [m, ldb >= D] fp32, la [n], lb [m] int64 labels, T > 0, l_ij = (a_i . b_j) / T (a division, as
// the reference's `matmul / temperature`).  Symmetric form: b absent, then b = a, lb = la and exclude_self may be set.
//     N_i   = all j (with exclude_self: all j != i)            P_i = { j in N_i : la[i] == lb[j] },  c_i = |P_i|
//     m_i   = max_j l_ij over ALL j (self included: the reference's logits_max)
//     lse_i = m_i + log(sum_{j in N_i} exp(l_ij - m_i) + 1e-10)
//     loss  = (scale / n) sum_i [ -(sum_{j in P_i} (l_ij - lse_i)) / (c_i + 1e-10) ]        (a row with c_i = 0 adds 0)
// Backward, p_ij = exp(l_ij - lse_i) recomputed:
//     q_ij  = [j in N_i] p_ij c_i / (c_i + 1e-10) - [j in P_i] / (c_i + 1e-10)
//     da_i  = coef sum_j q_ij b_j,   db_j = coef sum_i q_ij a_i,   coef = g scale / (n T);  symmetric: the one result da + db.
//
// Products: as softmax_ce.hip (split-bf16 operands, the count from rp_matmul_products, fp32-faithful 6 by default).
//
// Work split (a workgroup = 4 waves, every wave owns whole 32 x 32 tiles):
//   forward   grid (ceil(n / 32), splits of m).  The tile is formed transposed, S'[j, i] = B_tile . A_tile^T, so a lane holds 16
//             scores of ONE row i: running maximum, sum (online softmax, the self pair left out of the sum only), the count of
//             positives and the sum of their l_ij are per-lane registers; lane halves, waves and splits are merged in a fixed
//             order (ctr_finish_kernel: one thread per row walks the splits in ascending order), which leaves lse [n], c [n]
//             and per-workgroup sums of the row terms; st_mean_kernel adds those in a fixed order.
//   da        same grid, orientation and product order: q in registers is the next MFMA's B operand as it is; one [n, D] slab
//             per split, st_slab_reduce_kernel adds the slabs in split order (and, symmetric form, the db result) and scales.
//   db        grid ceil(m / 32): a workgroup owns 32 rows of b and walks all of a; the tile is S[i, j] (the same piece pairs in
//             the same order), the accumulator is the A operand; every row of db has one writer.
// No floating-point atomics: loss and gradients are bit-identical from run to run.
//
// Saved between forward and backward: lse [n] (float64: m_i + log(sum) added in double and split into hi + lo by the backward,
// so that p = exp((l - hi) - lo) keeps the digits of log(sum) beside m ~ 24) and c [n] (the count as a float).
// D: 1 .. ST_MAX_D = 128, zero-padded to 32 (score_tile.h's register budget); above, RP_ERR_ARG and nothing is launched.
#include "score_tile.h"

#define CTR_EPS 1e-10f

namespace {

// what one row knows of a range of columns: maximum over all of them, sum of exp(l - m) over N_i, |P_i| and the sum of l
// over P_i; m = -inf marks "nothing yet"
struct CtrStat {
    float m, l, ps;
    int cnt;
};

__device__ __forceinline__ void ctr_merge(CtrStat &x, const CtrStat &y) {
    const float mm = fmaxf(x.m, y.m);
    const float a = (x.m == -INFINITY) ? 0.f : expf(x.m - mm);
    const float b = (y.m == -INFINITY) ? 0.f : expf(y.m - mm);
    x.l = __fadd_rn(__fmul_rn(x.l, a), __fmul_rn(y.l, b));
    x.m = mm;
    x.ps = __fadd_rn(x.ps, y.ps);
    x.cnt += y.cnt;
}

template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void ctr_fwd_kernel(const float *__restrict__ A, int64_t lda,
                                                           const float *__restrict__ Bm, int64_t ldb,
                                                           const int64_t *__restrict__ la, const int64_t *__restrict__ lb,
                                                           int64_t n, int64_t m, int D, int64_t tps, int fastA, int fastB,
                                                           float T, int excl, float *__restrict__ part) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float sm[ST_WAVES][32], sl[ST_WAVES][32], sp[ST_WAVES][32];
    __shared__ int sc[ST_WAVES][32];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * ST_TILE;
    const StTiles tr = st_split_tiles(m, tps);
    const int64_t row = i0 + r;
    const bool ivalid = row < n;
    bf16x8 af[KS][NP];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(A, lda, row, ivalid, 16 * ks + 8 * h, D, fastA), af[ks]);
    const int64_t lab = ivalid ? la[row] : 0;
    CtrStat st;
    st.m = -INFINITY;
    st.l = 0.f;
    st.ps = 0.f;
    st.cnt = 0;
    for (int64_t t = tr.t0 + w; t < tr.t1; t += ST_WAVES) {
        const int64_t j0 = t * ST_TILE;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 bf[NP];
            bf_split8<NP>(st_load8(Bm, ldb, j0 + r, j0 + r < m, 16 * ks + 8 * h, D, fastB), bf);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[BfProd<NPROD>::pa(pr)], af[ks][BfProd<NPROD>::pb(pr)], acc, 0, 0, 0);
        }
        // acc[i] = a_row . b_j at j = j0 + rp_mfma32_row(i, h)
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[i] = (j0 + rp_mfma32_row(i, h) < m) ? __fdiv_rn(acc[i], T) : -INFINITY;
            tm = fmaxf(tm, acc[i]);
        }
        if (tm > -INFINITY) {
            const float mn = fmaxf(st.m, tm);
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t j = j0 + rp_mfma32_row(i, h);
                const bool in_n = j < m && !(excl && j == row);
                if (in_n) {
                    sum += expf(acc[i] - mn);
                    if (ivalid && lb[j] == lab) {
                        st.cnt += 1;
                        st.ps += acc[i];
                    }
                }
            }
            st.l = __fadd_rn(__fmul_rn(st.l, (st.m == -INFINITY) ? 0.f : expf(st.m - mn)), sum);
            st.m = mn;
        }
    }
    // the two lane halves hold different columns j of the same row
    CtrStat o;
    o.m = __shfl_xor(st.m, 32, 64);
    o.l = __shfl_xor(st.l, 32, 64);
    o.ps = __shfl_xor(st.ps, 32, 64);
    o.cnt = __shfl_xor(st.cnt, 32, 64);
    if (h == 0) {
        ctr_merge(st, o);
        sm[w][r] = st.m;
        sl[w][r] = st.l;
        sp[w][r] = st.ps;
        sc[w][r] = st.cnt;
    }
    __syncthreads();
    if (threadIdx.x < 32 && i0 + threadIdx.x < n) {
        const int x = threadIdx.x;
        CtrStat a;
        a.m = sm[0][x];
        a.l = sl[0][x];
        a.ps = sp[0][x];
        a.cnt = sc[0][x];
#pragma unroll
        for (int q = 1; q < ST_WAVES; ++q) {
            CtrStat b;
            b.m = sm[q][x];
            b.l = sl[q][x];
            b.ps = sp[q][x];
            b.cnt = sc[q][x];
            ctr_merge(a, b);
        }
        float *out = part + ((int64_t)blockIdx.y * n + i0 + x) * 4;
        out[0] = a.m;
        out[1] = a.l;
        out[2] = a.ps;
        out[3] = __int_as_float(a.cnt);
    }
}

// lse[i], c[i] and the workgroup's sum of the row terms: one thread per row walks the splits in ascending order
__global__ __launch_bounds__(ST_BLOCK) void ctr_finish_kernel(const float *__restrict__ part, int nsplit, int64_t n,
                                                              double *__restrict__ lse, float *__restrict__ c,
                                                              float *__restrict__ partial) {
    __shared__ float sh[ST_WAVES];
    const int64_t row = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x;
    float term = 0.f;
    if (row < n) {
        CtrStat a;
        a.m = -INFINITY;
        a.l = 0.f;
        a.ps = 0.f;
        a.cnt = 0;
        for (int s = 0; s < nsplit; ++s) {
            const float *p = part + ((int64_t)s * n + row) * 4;
            CtrStat b;
            b.m = p[0];
            b.l = p[1];
            b.ps = p[2];
            b.cnt = __float_as_int(p[3]);
            ctr_merge(a, b);
        }
        // (the sum in double: log(sum) of a row whose positive holds nearly all of its probability is ~1e-2 beside m ~ 24, and
        // the backward's q = p - 1 there is only as good as lse - m)
        const double v = (double)a.m + (double)logf(a.l + CTR_EPS);
        const float cf = (float)a.cnt;
        lse[row] = v;
        c[row] = cf;
        // sum_{j in P} (l_ij - lse) = ps - c lse
        if (a.cnt > 0) term = -(float)((double)a.ps - (double)cf * v) / (cf + CTR_EPS);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void ctr_da_kernel(const float *__restrict__ A, int64_t lda,
                                                          const float *__restrict__ Bm, int64_t ldb,
                                                          const int64_t *__restrict__ la, const int64_t *__restrict__ lb,
                                                          const double *__restrict__ lse, const float *__restrict__ c, int64_t n,
                                                          int64_t m, int D, int64_t tps, int fastA, int fastB, float T, int excl,
                                                          float *__restrict__ dAp) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float red[(ST_WAVES - 1) * DT * 16 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * ST_TILE;
    const StTiles tr = st_split_tiles(m, tps);
    const int64_t row = i0 + r;
    const bool ivalid = row < n;
    bf16x8 af[KS][NP];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(A, lda, row, ivalid, 16 * ks + 8 * h, D, fastA), af[ks]);
    const double lse_d = ivalid ? lse[row] : 0.0;
    const float lse_hi = (float)lse_d, lse_lo = (float)(lse_d - (double)lse_hi);  // l - hi is exact near the maximum
    const float c_i = ivalid ? c[row] : 0.f;
    const float w_i = c_i / (c_i + CTR_EPS), rc_i = 1.f / (c_i + CTR_EPS);
    const int64_t lab = ivalid ? la[row] : 0;
    f32x16 dacc[DT];  // dA^T[d = 32 dt + rp_mfma32_row(i, h), row]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dacc[dt][i] = 0.f;
    for (int64_t t = tr.t0 + w; t < tr.t1; t += ST_WAVES) {
        const int64_t j0 = t * ST_TILE;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 bf[NP];
            bf_split8<NP>(st_load8(Bm, ldb, j0 + r, j0 + r < m, 16 * ks + 8 * h, D, fastB), bf);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[BfProd<NPROD>::pa(pr)], af[ks][BfProd<NPROD>::pb(pr)], acc, 0, 0, 0);
        }
        // the forward's bits of a_row . b_j -> q_ij
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t j = j0 + rp_mfma32_row(i, h);
            float q = 0.f;
            if (ivalid && j < m && c_i > 0.f && !(excl && j == row)) {
                q = expf((__fdiv_rn(acc[i], T) - lse_hi) - lse_lo) * w_i;
                if (lb[j] == lab) q -= rc_i;
            }
            acc[i] = q;
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
                bf16x8 xf[NP];  // A operand[row d = 32 dt + r][k] = b[j0 + (row of k), d]
                bf_split8<NP>(st_load_rows(Bm, ldb, j0, m, s, h, 32 * dt + r, D), xf);
#pragma unroll
                for (int pr = 0; pr < NPROD; ++pr)
                    dacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[BfProd<NPROD>::pa(pr)], pf[BfProd<NPROD>::pb(pr)], dacc[dt],
                                                                       0, 0, 0);
            }
        }
    }
    st_add_waves<DT>(dacc, red, w, lane);
    if (w == 0 && ivalid) {
        float *o = dAp + ((int64_t)blockIdx.y * n + row) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int d = 32 * dt + rp_mfma32_row(i, h);
                if (d < D) o[d] = dacc[dt][i];
            }
    }
}

// gloss == nullptr: the unscaled sums (the symmetric form's second half, added by st_slab_reduce_kernel)
template <int DT, int NPROD>
__global__ __launch_bounds__(ST_BLOCK) void ctr_db_kernel(const float *__restrict__ A, int64_t lda,
                                                          const float *__restrict__ Bm, int64_t ldb,
                                                          const int64_t *__restrict__ la, const int64_t *__restrict__ lb,
                                                          const double *__restrict__ lse, const float *__restrict__ c,
                                                          const float *__restrict__ gloss, float coef, int64_t n, int64_t m,
                                                          int D, int fastA, int fastB, float T, int excl,
                                                          float *__restrict__ dB, int64_t lddb) {
    constexpr int NP = BfProd<NPROD>::NP;
    constexpr int KS = 2 * DT;
    __shared__ float red[(ST_WAVES - 1) * DT * 16 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * ST_TILE;
    const int64_t col = j0 + r;
    const bool jvalid = col < m;
    const int64_t itiles = (n + 31) / 32;
    bf16x8 bf[KS][NP];  // B operand[k][col r] = b[j0 + r, k]
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf_split8<NP>(st_load8(Bm, ldb, col, jvalid, 16 * ks + 8 * h, D, fastB), bf[ks]);
    const int64_t lab = jvalid ? lb[col] : 0;
    f32x16 zacc[DT];  // dB[j = j0 + rp_mfma32_row(i, h), d = 32 dt + r]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) zacc[dt][i] = 0.f;
    for (int64_t it = w; it < itiles; it += ST_WAVES) {
        const int64_t i0 = it * 32;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 af[NP];
            bf_split8<NP>(st_load8(A, lda, i0 + r, i0 + r < n, 16 * ks + 8 * h, D, fastA), af);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
                // (the forward pairs piece pa of b with piece pb of a: the same pairs in the same order here)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[BfProd<NPROD>::pb(pr)], bf[ks][BfProd<NPROD>::pa(pr)], acc, 0, 0, 0);
        }
        // acc[i] = a_row . b_col at row = i0 + rp_mfma32_row(i, h)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t row = i0 + rp_mfma32_row(i, h);
            float q = 0.f;
            if (jvalid && row < n && !(excl && row == col)) {
                const float c_i = c[row];
                if (c_i > 0.f) {
                    const double lse_d = lse[row];
                    const float lse_hi = (float)lse_d, lse_lo = (float)(lse_d - (double)lse_hi);
                    q = expf((__fdiv_rn(acc[i], T) - lse_hi) - lse_lo) * (c_i / (c_i + CTR_EPS));
                    if (la[row] == lab) q -= 1.f / (c_i + CTR_EPS);
                }
            }
            acc[i] = q;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f32x8 pv;
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = acc[8 * s + j];
            bf16x8 pf[NP];  // A operand[row j = r][k] = q[i0 + (row of k), j0 + r]
            bf_split8<NP>(pv, pf);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x8 xf[NP];  // B operand[k][col d = 32 dt + r] = a[i0 + (row of k), d]
                bf_split8<NP>(st_load_rows(A, lda, i0, n, s, h, 32 * dt + r, D), xf);
#pragma unroll
                for (int pr = 0; pr < NPROD; ++pr)
                    zacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[BfProd<NPROD>::pa(pr)], xf[BfProd<NPROD>::pb(pr)], zacc[dt],
                                                                       0, 0, 0);
            }
        }
    }
    st_add_waves<DT>(zacc, red, w, lane);
    if (w == 0) {
        const float scale = gloss ? gloss[0] * coef : 1.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = 32 * dt + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t j = j0 + rp_mfma32_row(i, h);
                if (j < m && d < D) dB[j * lddb + d] = zacc[dt][i] * scale;
            }
        }
    }
}

struct CtrWs {
    float *part, *partial, *dap, *dbt;
    size_t bytes;
};

// part [nsplit, n, 4] | partial [ceil(n / 256)] | dap [nsplit, n, D] | dbt [n, D] (the symmetric form's db, m == n there)
CtrWs ctr_workspace(void *base, int64_t n, int D, const StPlan &g) {
    CtrWs w;
    const size_t n_part = (size_t)4 * g.nsplit * n, n_partial = ((size_t)rp_cdiv(n, ST_BLOCK) + 3) & ~(size_t)3;
    const size_t n_dap = (((size_t)g.nsplit * n * D) + 3) & ~(size_t)3, n_dbt = (size_t)n * D;
    w.part = reinterpret_cast<float *>(base);
    w.partial = w.part + n_part;
    w.dap = w.partial + n_partial;
    w.dbt = w.dap + n_dap;
    w.bytes = (n_part + n_partial + n_dap + n_dbt) * sizeof(float);
    return w;
}

}  // namespace

extern "C" int rp_contrast_fits(int D) { return D >= 1 && D <= ST_MAX_D; }

extern "C" int rp_contrast_geometry(int *ta, int *tb, int *max_d, int *max_splits) {
    RP_REQUIRE(ta && tb && max_d && max_splits, "contrast_geometry: null pointer");
    *ta = ST_TILE;
    *tb = ST_TILE;
    *max_d = ST_MAX_D;
    *max_splits = ST_MAX_SPLITS;
    return RP_OK;
}

extern "C" int rp_contrast_workspace_bytes(int64_t n, int64_t m, int D, size_t *bytes) {
    RP_REQUIRE(bytes, "contrast_workspace_bytes: null pointer");
    RP_REQUIRE(n >= 1 && m >= 1 && D >= 1, "contrast_workspace_bytes: n, m and D must be positive");
    *bytes = ctr_workspace(nullptr, n, D, st_plan(n, m)).bytes;
    return RP_OK;
}

extern "C" int rp_contrast_fwd(const float *a, int64_t lda, const float *b, int64_t ldb, const int64_t *la, const int64_t *lb,
                               int64_t n, int64_t m, int D, float temperature, int exclude_self, float scale, double *lse,
                               float *c, float *loss, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(a && la && lse && c && loss && workspace, "contrast_fwd: null pointer");
    if (!b) {
        RP_REQUIRE(!lb || lb == la, "contrast_fwd: the symmetric form (b absent) takes no labels of b");
        b = a, ldb = lda, lb = la, m = n;
    } else {
        RP_REQUIRE(lb, "contrast_fwd: null pointer");
        RP_REQUIRE(!exclude_self, "contrast_fwd: exclude_self belongs to the symmetric form (b absent)");
    }
    RP_REQUIRE(n >= 1 && m >= 1 && D >= 1 && lda >= D && ldb >= D, "contrast_fwd: bad n / m / D / lda / ldb");
    RP_REQUIRE(D <= ST_MAX_D, "contrast_fwd: D=%d above the %d the register budget takes", D, ST_MAX_D);
    RP_REQUIRE(temperature > 0.f, "contrast_fwd: the temperature must be positive");
    const StPlan g = st_plan(n, m);
    const CtrWs ws = ctr_workspace(workspace, n, D, g);
    RP_REQUIRE(workspace_bytes >= ws.bytes && rp_aligned16(workspace), "contrast_fwd: workspace too small or misaligned");
    const int dt = (D + 31) / 32, nprod = st_products(n, m, D);
    const int fa = st_fast(a, lda, D), fb = st_fast(b, ldb, D);
    const int excl = exclude_self ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
#define CALL(DT_, NP_)                                                                                                      \
    hipLaunchKernelGGL((ctr_fwd_kernel<DT_, NP_>), dim3((unsigned)g.row_tiles, (unsigned)g.nsplit), dim3(ST_BLOCK), 0, s, a,  \
                       lda, b, ldb, la, lb, n, m, D, g.tps, fa, fb, temperature, excl, ws.part)
    ST_DISPATCH(dt, nprod, CALL);
#undef CALL
    RP_LAUNCH_CHECK("contrast_fwd");
    const int64_t nb = rp_cdiv(n, ST_BLOCK);
    hipLaunchKernelGGL(ctr_finish_kernel, dim3((unsigned)nb), dim3(ST_BLOCK), 0, s, ws.part, g.nsplit, n, lse, c, ws.partial);
    RP_LAUNCH_CHECK("contrast_finish");
    hipLaunchKernelGGL(st_mean_kernel, dim3(1), dim3(ST_BLOCK), 0, s, ws.partial, nb, scale / (float)n, loss);
    RP_LAUNCH_CHECK("contrast_mean");
    return RP_OK;
}

extern "C" int rp_contrast_bwd(const float *a, int64_t lda, const float *b, int64_t ldb, const int64_t *la, const int64_t *lb,
                               const double *lse, const float *c, const float *gloss, int64_t n, int64_t m, int D,
                               float temperature, int exclude_self, float scale, float *da, int64_t ldda, float *db, int64_t lddb,
                               void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(a && la && lse && c && gloss && workspace, "contrast_bwd: null pointer");
    const bool sym = !b;
    if (sym) {
        RP_REQUIRE(!lb || lb == la, "contrast_bwd: the symmetric form (b absent) takes no labels of b");
        RP_REQUIRE(da && !db, "contrast_bwd: the symmetric form has the one gradient da");
        b = a, ldb = lda, lb = la, m = n;
    } else {
        RP_REQUIRE(lb, "contrast_bwd: null pointer");
        RP_REQUIRE(!exclude_self, "contrast_bwd: exclude_self belongs to the symmetric form (b absent)");
        RP_REQUIRE(da || db, "contrast_bwd: neither gradient asked for");
    }
    RP_REQUIRE(n >= 1 && m >= 1 && D >= 1 && lda >= D && ldb >= D && (!da || ldda >= D) && (!db || lddb >= D),
               "contrast_bwd: bad n / m / D / leading dimensions");
    RP_REQUIRE(D <= ST_MAX_D, "contrast_bwd: D=%d above the %d the register budget takes", D, ST_MAX_D);
    RP_REQUIRE(temperature > 0.f, "contrast_bwd: the temperature must be positive");
    const StPlan g = st_plan(n, m);
    const CtrWs ws = ctr_workspace(workspace, n, D, g);
    RP_REQUIRE(workspace_bytes >= ws.bytes && rp_aligned16(workspace), "contrast_bwd: workspace too small or misaligned");
    const int dt = (D + 31) / 32, nprod = st_products(n, m, D);
    const int fa = st_fast(a, lda, D), fb = st_fast(b, ldb, D);
    const int excl = exclude_self ? 1 : 0;
    const float coef = scale / ((float)n * temperature);
    hipStream_t s = (hipStream_t)stream;
    if (db || sym) {
        float *out = sym ? ws.dbt : db;
        const int64_t ldo = sym ? (int64_t)D : lddb;
        const float *gl = sym ? nullptr : gloss;
#define CALL(DT_, NP_)                                                                                                       \
    hipLaunchKernelGGL((ctr_db_kernel<DT_, NP_>), dim3((unsigned)g.tiles), dim3(ST_BLOCK), 0, s, a, lda, b, ldb, la, lb, lse, c,  \
                       gl, coef, n, m, D, fa, fb, temperature, excl, out, ldo)
        ST_DISPATCH(dt, nprod, CALL);
#undef CALL
        RP_LAUNCH_CHECK("contrast_db");
    }
    if (da) {
#define CALL(DT_, NP_)                                                                                                     \
    hipLaunchKernelGGL((ctr_da_kernel<DT_, NP_>), dim3((unsigned)g.row_tiles, (unsigned)g.nsplit), dim3(ST_BLOCK), 0, s, a,  \
                       lda, b, ldb, la, lb, lse, c, n, m, D, g.tps, fa, fb, temperature, excl, ws.dap)
        ST_DISPATCH(dt, nprod, CALL);
#undef CALL
        RP_LAUNCH_CHECK("contrast_da");
        int64_t nb = rp_cdiv(n * D, ST_BLOCK);
        if (nb > 4096) nb = 4096;
        const float *extra = sym ? ws.dbt : nullptr;
        hipLaunchKernelGGL(st_slab_reduce_kernel, dim3((unsigned)nb), dim3(ST_BLOCK), 0, s, ws.dap, g.nsplit, n, D, extra, gloss,
                           coef, da, ldda);
        RP_LAUNCH_CHECK("contrast_da_reduce");
    }
    return RP_OK;
}
