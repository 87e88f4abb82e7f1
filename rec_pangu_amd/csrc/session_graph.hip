// Session graphs and their gated graph cell, gfx950 — replaces generate_graph of rec_pangu/models/utils.py (a Python loop over
// the batch with torch.unique, two dgl graphs) and SRGNNConv / SRGNNCell of rec_pangu/models/layers/graph.py (dgl message
// passing) with their autograd, for SRGNN, NISER and GCSAN.  Also the row-wise L2 normalisation NISER applies twice.
//
// LAYOUT.  A session of at most L items has at most L distinct items: sample b keeps its nodes in its own L slots, node v is
// row b L + v of a [B, L, D] tensor, rows behind the node count are zero.  No offsets between graphs, no prefix sum over the
// batch, and every stage has the [B, L, D] shape of the other sequence kernels.  The graph itself is the alias list alone
// (int32 [B, L]: the node of the l-th item with id > 0, -1 behind them): transition l is alias[l] -> alias[l + 1], and the
// cell counts lengths, node counts and degrees from it while it loads its tile.
//
// rp_session_graph: a wave per sample, a lane per position.  The items with id > 0 are compacted by a ballot; a lane's node
//   number is the count of smaller FIRST occurrences among them (what torch.unique's ascending order gives); degrees are
//   counts over the alias list.  Integer work only.
//
// rp_ggnn_cell_fwd: a workgroup of 256 threads owns TS samples (TS L <= 64 rows, padded to 32); in LDS the node tile H, one
//   projection tile P and the aggregate tile [in | out].  Stages: P = H W_in^T + b_in, in[v] = sum over the transitions that
//   end in v, in position order, of P[u] / outdeg(u); the same with W_out for out[u] = sum P[v] / indeg(v); then ONE product
//   loop per 32 x 32 output tile with four accumulators (r and z summed over lin_ih and lin_hh, i_n and h_n apart), the gates
//   and the blend in registers.  All products run on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32) against zero-padded
//   copies of the weights in the workspace (one small launch per call), read through L2.  The final step also reads the
//   result back in sequence order (seq_hidden, ht) from the tile.  No [B L, 3 D] tensor exists in the forward.
//
// rp_ggnn_cell_bwd: one launch recomputes the stages from the step's input, takes the three arriving gradients as ONE tile
//   (dHout + the positions of dseq that name the node, in position order, + dht at the last position's node), forms the
//   pre-activation gradients in the gate epilogue and leaves them, with the aggregate tile and the two projections'
//   gradients, as stacked rows in the workspace; their products with the transposed weights run from there (the rows a
//   workgroup reads are its own).  Both reverse aggregations GATHER.  dW and db of the four Linears are then one
//   rp_linear_wgrad each over the stacked rows.  No floating-point atomics: two runs give the same bits.
#include "common.h"

namespace {

constexpr int SG_MAX_L = 64, SG_MAX_D = 128;
constexpr size_t SG_LDS_MAX = 160 * 1024 - 512;
constexpr float SG_L2_EPS = 1e-12f;

// ---------------------------------------------------------------------------------------------------------------------------
// the graph
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sg_graph_kernel(const int64_t *__restrict__ hist, int64_t B, int L, int64_t *__restrict__ nodes,
                                                       int32_t *__restrict__ alias, int32_t *__restrict__ count,
                                                       int32_t *__restrict__ indeg, int32_t *__restrict__ outdeg) {
    __shared__ int64_t sid[4][64], snode[4][64];
    __shared__ int sfirst[4][64], sal[4][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + w;
    const bool in = b < B && lane < L;
    const int64_t id = in ? hist[b * L + lane] : 0;
    const bool valid = id > 0;
    const unsigned long long m = __ballot(valid);
    const int p = __popcll(m & ((1ull << lane) - 1ull)), n = __popcll(m);
    if (valid) sid[w][p] = id;
    snode[w][lane] = 0;
    __syncthreads();
    int64_t my = 0;
    bool first = false;
    if (lane < n) {
        my = sid[w][lane];
        first = true;
        for (int k = 0; k < lane; ++k) first = first && sid[w][k] != my;
    }
    sfirst[w][lane] = first;
    const int cnt = __popcll(__ballot(first));
    __syncthreads();
    int rank = -1;
    if (lane < n) {
        rank = 0;
        for (int j = 0; j < n; ++j) rank += (sfirst[w][j] && sid[w][j] < my) ? 1 : 0;
    }
    sal[w][lane] = rank;
    if (first) snode[w][rank] = my;
    __syncthreads();
    if (!in) return;
    int od = 0, idg = 0;
    if (lane < cnt) {
        for (int l = 0; l < n; ++l) {
            if (sal[w][l] != lane) continue;
            od += l < n - 1, idg += l > 0;
        }
    }
    nodes[b * L + lane] = snode[w][lane];
    alias[b * L + lane] = rank;
    indeg[b * L + lane] = idg;
    outdeg[b * L + lane] = od;
    if (lane == 0) count[b] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------------------
// L2 normalisation of rows: a wave per row
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sg_l2norm_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t M, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = x[row * D + c];
        s += v * v;
    }
    const float inv = 1.f / fmaxf(sqrtf(rp_lane_sum(s)), SG_L2_EPS);
    for (int c = lane; c < D; c += 64) y[row * D + c] = x[row * D + c] * inv;
}

// dx = dy / n - x (x . dy) / n^3 for n = |x| >= eps; dy / eps below it (the clamp passes nothing to the norm); 0 for a zero row
__global__ __launch_bounds__(256) void sg_l2norm_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                            float *__restrict__ dx, int64_t M, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float s = 0.f, t = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = x[row * D + c];
        s += v * v, t += v * dy[row * D + c];
    }
    s = rp_lane_sum(s), t = rp_lane_sum(t);
    const float nrm = sqrtf(s);
    float a = 0.f, bq = 0.f;  // dx = a dy - bq x
    if (nrm >= SG_L2_EPS) a = 1.f / nrm, bq = t / (nrm * s);
    else if (nrm > 0.f) a = 1.f / SG_L2_EPS;
    for (int c = lane; c < D; c += 64) dx[row * D + c] = a * dy[row * D + c] - bq * x[row * D + c];
}

// ---------------------------------------------------------------------------------------------------------------------------
// the cell
// ---------------------------------------------------------------------------------------------------------------------------
struct GgArgs {
    const float *H;        // [B, L, D] the step's input
    const int32_t *alias;  // [B, L]
    const float *dHout, *dseq, *dht;  // [B, L, D], [B, L, D], [B, D]: each may be NULL
    float *Hout, *seq, *ht, *dH;      // forward outputs (each may be NULL), backward output
    int64_t B, nwg;
    int L, D, Wp, ld, ld2, TS, Mv, Mp, s3, K3p;
    const float *w[4], *bias[4];  // incomming_conv.lin, outcomming_conv.lin, lin_ih, lin_hh
    float *wP[4];  // forward forms: [Wp][Wp], [Wp][Wp], [3 Wp][2 Wp] (column Wp + k reads input D + k), [3 Wp][Wp]
    float *wT[4];  // transposed forms: [Wp][Wp], [Wp][Wp], [2 Wp][K3p], [Wp][K3p] (gate g's row c at column g D + c)
    float *AGG, *dGI, *dGH, *dP[2];  // stacked rows: [B L, 2 D], [B L, s3], [B L, s3], [B L, D] each
};

__global__ __launch_bounds__(256) void gg_pack_kernel(GgArgs a, int backward) {
    const int D = a.D, Wp = a.Wp, gstride = gridDim.x * 256, g0 = blockIdx.x * 256 + threadIdx.x;
    for (int q = 0; q < 2; ++q)
        for (int idx = g0; idx < Wp * Wp; idx += gstride) {
            const int k = idx % Wp, c = idx / Wp;
            a.wP[q][idx] = (c < D && k < D) ? a.w[q][c * D + k] : 0.f;
            if (backward) a.wT[q][idx] = (c < D && k < D) ? a.w[q][k * D + c] : 0.f;
        }
    for (int idx = g0; idx < 3 * Wp * 2 * Wp; idx += gstride) {
        const int k = idx % (2 * Wp), r = idx / (2 * Wp), g = r / Wp, c = r % Wp;
        const int kk = k < Wp ? k : k - Wp;
        a.wP[2][idx] = (c < D && kk < D) ? a.w[2][(int64_t)(g * D + c) * 2 * D + (k < Wp ? kk : D + kk)] : 0.f;
    }
    for (int idx = g0; idx < 3 * Wp * Wp; idx += gstride) {
        const int k = idx % Wp, r = idx / Wp, g = r / Wp, c = r % Wp;
        a.wP[3][idx] = (c < D && k < D) ? a.w[3][(int64_t)(g * D + c) * D + k] : 0.f;
    }
    if (!backward) return;
    for (int idx = g0; idx < 2 * Wp * a.K3p; idx += gstride) {
        const int k = idx % a.K3p, c2 = idx / a.K3p, cc = c2 < Wp ? c2 : c2 - Wp;
        a.wT[2][idx] = (k < 3 * D && cc < D) ? a.w[2][(int64_t)k * 2 * D + (c2 < Wp ? cc : D + cc)] : 0.f;
    }
    for (int idx = g0; idx < Wp * a.K3p; idx += gstride) {
        const int k = idx % a.K3p, c = idx / a.K3p;
        a.wT[3][idx] = (k < 3 * D && c < D) ? a.w[3][(int64_t)k * D + c] : 0.f;
    }
}

// the workgroup's tables
struct GgTile {
    float *HB, *PB, *AG;  // [Mp][ld], [Mp][ld], [Mp][ld2]
    int *sal;             // [Mp] alias of position l of sample s at s L + l (-1: none)
    int *grow;            // [Mp] global row b L + v of tile row s L + v (-1: no such sample)
    int *nn, *cn;         // [Mp] the sample's item count and node count
    float *iod, *iid;     // [Mp] 1 / outdeg, 1 / indeg of the node (0 where the degree is 0)
};

__device__ __forceinline__ GgTile gg_carve(const GgArgs &a, float *lds) {
    GgTile t;
    t.HB = lds, t.PB = t.HB + a.Mp * a.ld, t.AG = t.PB + a.Mp * a.ld;
    t.sal = reinterpret_cast<int *>(t.AG + a.Mp * a.ld2);
    t.grow = t.sal + a.Mp, t.nn = t.grow + a.Mp, t.cn = t.nn + a.Mp;
    t.iod = reinterpret_cast<float *>(t.cn + a.Mp), t.iid = t.iod + a.Mp;
    return t;
}

__device__ __forceinline__ void gg_tables(const GgArgs &a, const GgTile &t, int64_t b0) {
    for (int m = threadIdx.x; m < a.Mp; m += blockDim.x) {
        const int s = m / a.L, v = m % a.L;
        const int64_t b = b0 + s;
        int al = -1, gr = -1, n = 0, cnt = 0, od = 0, idg = 0;
        if (m < a.Mv && b < a.B) {
            const int32_t *row = a.alias + b * a.L;
            gr = (int)(b * a.L + v);
            int prev = -1;
            for (int l = 0; l < a.L; ++l) {
                int q = row[l];
                if (q < 0 || q >= a.L) break;  // (the list is a prefix; a value outside the sample's slots ends it)
                n = l + 1;
                cnt = q + 1 > cnt ? q + 1 : cnt;
                if (prev == v) ++od;           // transition l - 1 leaves v
                if (l > 0 && q == v) ++idg;    // transition l - 1 ends in v
                prev = q;
            }
            al = v < n ? row[v] : -1;
        }
        t.sal[m] = al, t.grow[m] = gr, t.nn[m] = n, t.cn[m] = cnt;
        t.iod[m] = od > 0 ? 1.f / (float)od : 0.f, t.iid[m] = idg > 0 ? 1.f / (float)idg : 0.f;
    }
}

__device__ __forceinline__ void gg_load_h(const GgArgs &a, const GgTile &t) {
    for (int idx = threadIdx.x; idx < a.Mp * a.Wp; idx += blockDim.x) {
        const int m = idx / a.Wp, c = idx % a.Wp;
        const int gr = t.grow[m];
        t.HB[m * a.ld + c] = (gr >= 0 && c < a.D && m % a.L < t.cn[m]) ? a.H[(int64_t)gr * a.D + c] : 0.f;
    }
}

// dst [Mp][Wp] (+)= src [Mp][Wp] . W^T (+ bias), W as [Wp][Wp] rows of the output column; tiles of LDS with row stride ld
__device__ __forceinline__ void gg_linear(const GgArgs &a, const float *src, float *dst, const float *__restrict__ W,
                                          const float *__restrict__ bias, bool accumulate) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int nrt = a.Mp / 32, ntile = nrt * (a.Wp / 32);
    for (int tile = w; tile < ntile; tile += nw) {
        const int rt = tile % nrt, ct = tile / nrt, col = ct * 32 + i;
        f32x16 acc = {0};
        if (accumulate) {
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = dst[(rt * 32 + rp_mfma32_row(q, h)) * a.ld + col];
        }
        acc = rp_mma_f32_rows(acc, src + (rt * 32 + i) * a.ld, a.Wp, a.Wp, W + (int64_t)col * a.Wp, h);
        const float bv = (bias != nullptr && col < a.D) ? bias[col] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) dst[(rt * 32 + rp_mfma32_row(q, h)) * a.ld + col] = acc[q] + bv;
    }
}

// dst[s L + v, c] = sum over the transitions l of the sample, in position order, whose end (tgt 1) or start (tgt 0) is v, of
// src[the other node, c] times wgt[the other node] (on_src) or wgt[v]; zero rows behind the node count and zero columns
// [D, Wp).  spill != NULL also keeps the D columns at spill[grow, spill_off + c] (row stride spill_ld).
__device__ __forceinline__ void gg_aggregate(const GgArgs &a, const GgTile &t, const float *src, int lds_src, float *dst, int lds_dst,
                                             int tgt, const float *wgt, bool on_src, float *__restrict__ spill, int spill_ld,
                                             int spill_off) {
    for (int idx = threadIdx.x; idx < a.Mp * a.Wp; idx += blockDim.x) {
        const int m = idx / a.Wp, c = idx % a.Wp;
        const int s = m / a.L, v = m % a.L, base = s * a.L;
        float acc = 0.f;
        if (m < a.Mv && c < a.D && v < t.cn[m]) {
            const int n = t.nn[m];
            for (int l = 0; l + 1 < n; ++l) {
                const int at = t.sal[base + l + tgt];
                if (at != v) continue;
                const int other = base + t.sal[base + l + 1 - tgt];
                acc += src[other * lds_src + c] * (on_src ? wgt[other] : wgt[m]);
            }
        }
        dst[m * lds_dst + c] = acc;
        if (spill != nullptr && c < a.D && t.grow[m] >= 0) spill[(int64_t)t.grow[m] * spill_ld + spill_off + c] = acc;
    }
}

// H -> P -> [in | out] in AG; KEEP: the aggregate's rows go to a.AGG
template <bool KEEP>
__device__ __forceinline__ void gg_front(const GgArgs &a, const GgTile &t) {
    gg_load_h(a, t);
    __syncthreads();
    gg_linear(a, t.HB, t.PB, a.wP[0], a.bias[0], false);
    __syncthreads();
    gg_aggregate(a, t, t.PB, a.ld, t.AG, a.ld2, 1, t.iod, true, KEEP ? a.AGG : nullptr, 2 * a.D, 0);
    __syncthreads();
    gg_linear(a, t.HB, t.PB, a.wP[1], a.bias[1], false);
    __syncthreads();
    gg_aggregate(a, t, t.PB, a.ld, t.AG + a.Wp, a.ld2, 0, t.iid, true, KEEP ? a.AGG : nullptr, 2 * a.D, a.D);
    __syncthreads();
}

// the gates of every element of the tile: BWD false -> PB = h'; BWD true -> PB holds dh' on entry and dh' (1 - z) on exit,
// the pre-activation gradients go to a.dGI / a.dGH
template <bool BWD>
__device__ __forceinline__ void gg_gates(const GgArgs &a, const GgTile &t) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int nrt = a.Mp / 32, ntile = nrt * (a.Wp / 32), D = a.D, Wp = a.Wp;
    const float *bih = a.bias[2], *bhh = a.bias[3];
    for (int tile = w; tile < ntile; tile += nw) {
        const int rt = tile % nrt, ct = tile / nrt, col = ct * 32 + i;
        const float *ag = t.AG + (rt * 32 + i) * a.ld2, *hb = t.HB + (rt * 32 + i) * a.ld;
        f32x16 ar = {0}, az = {0}, ani = {0}, anh = {0};
        ar = rp_mma_f32_rows(ar, ag, 2 * Wp, 2 * Wp, a.wP[2] + (int64_t)(0 * Wp + col) * 2 * Wp, h);
        az = rp_mma_f32_rows(az, ag, 2 * Wp, 2 * Wp, a.wP[2] + (int64_t)(1 * Wp + col) * 2 * Wp, h);
        ani = rp_mma_f32_rows(ani, ag, 2 * Wp, 2 * Wp, a.wP[2] + (int64_t)(2 * Wp + col) * 2 * Wp, h);
        ar = rp_mma_f32_rows(ar, hb, Wp, Wp, a.wP[3] + (int64_t)(0 * Wp + col) * Wp, h);
        az = rp_mma_f32_rows(az, hb, Wp, Wp, a.wP[3] + (int64_t)(1 * Wp + col) * Wp, h);
        anh = rp_mma_f32_rows(anh, hb, Wp, Wp, a.wP[3] + (int64_t)(2 * Wp + col) * Wp, h);
        const bool cok = col < D;
        const float br = cok ? bih[col] + bhh[col] : 0.f, bz = cok ? bih[D + col] + bhh[D + col] : 0.f;
        const float bni = cok ? bih[2 * D + col] : 0.f, bnh = cok ? bhh[2 * D + col] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = rt * 32 + rp_mfma32_row(q, h);
            const bool live = cok && m < a.Mv && m % a.L < t.cn[m];
            const float r = rp_sigmoid(ar[q] + br), z = rp_sigmoid(az[q] + bz), hn = anh[q] + bnh;
            const float nv = tanhf(ani[q] + bni + r * hn), hv = t.HB[m * a.ld + col];
            if (!BWD) {
                t.PB[m * a.ld + col] = live ? (1.f - z) * hv + z * nv : 0.f;
            } else {
                const float dh = live ? t.PB[m * a.ld + col] : 0.f;
                const float dnp = dh * z * (1.f - nv * nv), dzp = dh * (nv - hv) * z * (1.f - z), drp = dnp * hn * r * (1.f - r);
                t.PB[m * a.ld + col] = dh * (1.f - z);
                const int gr = t.grow[m];
                if (cok && gr >= 0) {
                    float *gi = a.dGI + (int64_t)gr * a.s3, *gh = a.dGH + (int64_t)gr * a.s3;
                    gi[col] = drp, gi[D + col] = dzp, gi[2 * D + col] = dnp;
                    gh[col] = drp, gh[D + col] = dzp, gh[2 * D + col] = dnp * r;
                }
            }
        }
    }
}

// dynamic LDS: HB, PB [Mp][ld], AG [Mp][ld2] floats, sal / grow / nn / cn [Mp] ints, iod / iid [Mp] floats
__global__ __launch_bounds__(256) void gg_fwd_kernel(GgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gg_lds[];
    const GgTile t = gg_carve(a, gg_lds);
    const int64_t b0 = (int64_t)blockIdx.x * a.TS;
    gg_tables(a, t, b0);
    __syncthreads();
    gg_front<false>(a, t);
    gg_gates<false>(a, t);
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.Mv * a.D; idx += blockDim.x) {
        const int m = idx / a.D, c = idx % a.D, s = m / a.L;
        const int gr = t.grow[m];
        if (gr < 0) continue;
        if (a.Hout != nullptr) a.Hout[(int64_t)gr * a.D + c] = t.PB[m * a.ld + c];
        if (a.seq != nullptr) {  // (tile row s L + l doubles as position l of the sample)
            const int al = t.sal[m];
            a.seq[(int64_t)gr * a.D + c] = al >= 0 ? t.PB[(s * a.L + al) * a.ld + c] : 0.f;
        }
        if (a.ht != nullptr && m % a.L == 0) {
            const int n = t.nn[m];
            a.ht[(int64_t)(gr / a.L) * a.D + c] = n > 0 ? t.PB[(s * a.L + t.sal[s * a.L + n - 1]) * a.ld + c] : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void gg_bwd_kernel(GgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gg_lds[];
    const GgTile t = gg_carve(a, gg_lds);
    const int64_t b0 = (int64_t)blockIdx.x * a.TS;
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int D = a.D, Wp = a.Wp, L = a.L;
    gg_tables(a, t, b0);
    __syncthreads();
    gg_front<true>(a, t);
    // the arriving gradients as one tile: dHout, the positions of dseq that name the node (position order), dht
    for (int idx = threadIdx.x; idx < a.Mp * Wp; idx += blockDim.x) {
        const int m = idx / Wp, c = idx % Wp, s = m / L, v = m % L;
        const int gr = t.grow[m];
        float g = 0.f;
        if (gr >= 0 && c < D && v < t.cn[m]) {
            const int n = t.nn[m];
            const int64_t brow = (int64_t)(gr - v);  // b L
            if (a.dHout != nullptr) g = a.dHout[(int64_t)gr * D + c];
            if (a.dseq != nullptr)
                for (int l = 0; l < n; ++l)
                    if (t.sal[s * L + l] == v) g += a.dseq[(brow + l) * D + c];
            if (a.dht != nullptr && n > 0 && t.sal[s * L + n - 1] == v) g += a.dht[(brow / L) * D + c];
        }
        t.PB[m * a.ld + c] = g;
    }
    // the pad columns [3 D, s3) of the stacked gate gradients
    for (int idx = threadIdx.x; idx < a.Mv * (a.s3 - 3 * D); idx += blockDim.x) {
        const int m = idx / (a.s3 - 3 * D), c = 3 * D + idx % (a.s3 - 3 * D);
        if (t.grow[m] >= 0) a.dGI[(int64_t)t.grow[m] * a.s3 + c] = 0.f, a.dGH[(int64_t)t.grow[m] * a.s3 + c] = 0.f;
    }
    __syncthreads();
    gg_gates<true>(a, t);
    __syncthreads();  // (dGI / dGH rows of this workgroup are visible to it; AG and HB are free)
    // AG = dGI . W_ih (the gradient of [in | out]) and PB += dGH . W_hh, from the workgroup's own stacked rows
    {
        const int nrt = a.Mp / 32, nct = 3 * Wp / 32, ntile = nrt * nct;
        for (int tile = w; tile < ntile; tile += nw) {
            const int rt = tile % nrt, ct = tile / nrt, m = rt * 32 + i;
            const int gr = t.grow[m];
            const bool to_ag = ct < 2 * Wp / 32;
            const int col = (to_ag ? ct : ct - 2 * Wp / 32) * 32 + i;  // of AG [.., 2 Wp] or of PB [.., Wp]: the row of wT too
            float *dst = to_ag ? t.AG : t.PB;
            const int ldd = to_ag ? a.ld2 : a.ld;
            const float *arow = gr < 0 ? nullptr : (to_ag ? a.dGI : a.dGH) + (int64_t)gr * a.s3;
            f32x16 acc = {0};
            if (!to_ag) {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = dst[(rt * 32 + rp_mfma32_row(q, h)) * ldd + col];
            }
            acc = rp_mma_f32_rows(acc, arow, a.K3p, a.s3, a.wT[to_ag ? 2 : 3] + (int64_t)col * a.K3p, h);
#pragma unroll
            for (int q = 0; q < 16; ++q) dst[(rt * 32 + rp_mfma32_row(q, h)) * ldd + col] = acc[q];
        }
    }
    __syncthreads();
    // dP_in[u] = (sum over the transitions that leave u of d in[their end]) / outdeg(u);  PB += dP_in . W_in
    gg_aggregate(a, t, t.AG, a.ld2, t.HB, a.ld, 0, t.iod, false, a.dP[0], D, 0);
    __syncthreads();
    gg_linear(a, t.HB, t.PB, a.wT[0], nullptr, true);
    __syncthreads();
    // dP_out[v] = (sum over the transitions that end in v of d out[their start]) / indeg(v);  PB += dP_out . W_out
    gg_aggregate(a, t, t.AG + Wp, a.ld2, t.HB, a.ld, 1, t.iid, false, a.dP[1], D, 0);
    __syncthreads();
    gg_linear(a, t.HB, t.PB, a.wT[1], nullptr, true);
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.Mv * D; idx += blockDim.x) {
        const int m = idx / D, c = idx % D;
        if (t.grow[m] >= 0) a.dH[(int64_t)t.grow[m] * D + c] = t.PB[m * a.ld + c];
    }
}

bool gg_dims_ok(int L, int D) { return L >= 1 && L <= SG_MAX_L && D >= 1 && D <= SG_MAX_D; }

void gg_shape(int64_t B, int L, int D, GgArgs *a) {
    memset(a, 0, sizeof(*a));
    a->B = B, a->L = L, a->D = D;
    a->Wp = (int)rp_round_up(D, 32), a->ld = a->Wp + 4, a->ld2 = 2 * a->Wp + 4;
    a->TS = 64 / L, a->Mv = a->TS * L, a->Mp = (int)rp_round_up(a->Mv, 32);
    a->s3 = (int)rp_round_up(3 * D, 4), a->K3p = (int)rp_round_up(a->s3, 8);
    a->nwg = rp_cdiv(B, a->TS);
}

size_t gg_lds_bytes(const GgArgs &a) { return 4 * (size_t)a.Mp * (2 * a.ld + a.ld2 + 6); }

struct GgWs {
    size_t wP[4], wT[4], AGG, dGI, dGH, dP[2], wgrad, wgrad_bytes, total;
};

int gg_ws(const GgArgs &a, bool bwd, GgWs *o) {
    memset(o, 0, sizeof(*o));
    size_t off = 0;
    const size_t Wp = a.Wp, rows = (size_t)a.B * a.L, D = a.D;
    const size_t np[4] = {Wp * Wp, Wp * Wp, 6 * Wp * Wp, 3 * Wp * Wp}, nt[4] = {Wp * Wp, Wp * Wp, 2 * Wp * a.K3p, Wp * a.K3p};
    for (int q = 0; q < 4; ++q) o->wP[q] = off, off += rp_round_up(4 * np[q], 256);
    if (bwd) {
        for (int q = 0; q < 4; ++q) o->wT[q] = off, off += rp_round_up(4 * nt[q], 256);
        o->AGG = off, off += rp_round_up(4 * rows * 2 * D, 256);
        o->dGI = off, off += rp_round_up(4 * rows * a.s3, 256);
        o->dGH = off, off += rp_round_up(4 * rows * a.s3, 256);
        for (int q = 0; q < 2; ++q) o->dP[q] = off, off += rp_round_up(4 * rows * D, 256);
        const int N[4] = {a.D, a.D, 3 * a.D, 3 * a.D}, K[4] = {a.D, a.D, 2 * a.D, a.D};
        for (int q = 0; q < 4 && rows > 0; ++q) {
            size_t wb = 0;
            const int rc = rp_linear_wgrad_workspace_bytes((int64_t)rows, N[q], K[q], &wb);
            if (rc != RP_OK) return rc;
            o->wgrad_bytes = wb > o->wgrad_bytes ? wb : o->wgrad_bytes;
        }
        o->wgrad = off, off += rp_round_up(o->wgrad_bytes, 256);
    }
    o->total = off;
    return RP_OK;
}

#define GG_CHECK_DIMS(what)                                                                                                    \
    RP_REQUIRE(B >= 0 && gg_dims_ok(L, D), what ": need B >= 0, 1 <= L <= %d, 1 <= D <= %d (got B=%lld L=%d D=%d)", SG_MAX_L,  \
               SG_MAX_D, (long long)B, L, D);                                                                                  \
    RP_REQUIRE(B * (int64_t)L < ((int64_t)1 << 31) / 4, what ": B L must stay below 2^29")

int gg_bind(GgArgs *a, const float *const *params, void *workspace, const GgWs &ws, bool bwd, const char *what) {
    char *base = static_cast<char *>(workspace);
    for (int q = 0; q < 4; ++q) {
        RP_REQUIRE(params[2 * q] && params[2 * q + 1], "%s: null parameter", what);
        a->w[q] = params[2 * q], a->bias[q] = params[2 * q + 1];
        a->wP[q] = reinterpret_cast<float *>(base + ws.wP[q]);
        if (bwd) a->wT[q] = reinterpret_cast<float *>(base + ws.wT[q]);
    }
    if (bwd) {
        a->AGG = reinterpret_cast<float *>(base + ws.AGG);
        a->dGI = reinterpret_cast<float *>(base + ws.dGI), a->dGH = reinterpret_cast<float *>(base + ws.dGH);
        a->dP[0] = reinterpret_cast<float *>(base + ws.dP[0]), a->dP[1] = reinterpret_cast<float *>(base + ws.dP[1]);
    }
    return RP_OK;
}

}  // namespace

extern "C" int rp_session_graph_geometry(int *max_l, int *samples_per_workgroup) {
    RP_REQUIRE(max_l && samples_per_workgroup, "session_graph_geometry: null pointer");
    *max_l = SG_MAX_L, *samples_per_workgroup = 4;
    return RP_OK;
}

extern "C" int rp_session_graph(const int64_t *hist, int64_t B, int L, int64_t *nodes, int32_t *alias, int32_t *count,
                                int32_t *indeg, int32_t *outdeg, rp_stream_t stream) {
    RP_REQUIRE(B >= 0 && L >= 1 && L <= SG_MAX_L, "session_graph: need B >= 0 and 1 <= L <= %d (got B=%lld L=%d)", SG_MAX_L,
               (long long)B, L);
    RP_REQUIRE(B * (int64_t)L < ((int64_t)1 << 31), "session_graph: B L must stay below 2^31");
    RP_REQUIRE(hist && nodes && alias && count && indeg && outdeg, "session_graph: null pointer");
    if (B == 0) return RP_OK;
    hipLaunchKernelGGL(sg_graph_kernel, dim3((unsigned)rp_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, hist, B, L, nodes, alias,
                       count, indeg, outdeg);
    RP_LAUNCH_CHECK("session_graph");
    return RP_OK;
}

extern "C" int rp_l2norm_fwd(const float *x, float *y, int64_t M, int D, rp_stream_t stream) {
    RP_REQUIRE(M >= 0 && D >= 1 && M < ((int64_t)1 << 33), "l2norm_fwd: need M >= 0 and D >= 1");
    RP_REQUIRE(x && y, "l2norm_fwd: null pointer");
    if (M == 0) return RP_OK;
    hipLaunchKernelGGL(sg_l2norm_fwd_kernel, dim3((unsigned)rp_cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x, y, M, D);
    RP_LAUNCH_CHECK("l2norm_fwd");
    return RP_OK;
}

extern "C" int rp_l2norm_bwd(const float *x, const float *dy, float *dx, int64_t M, int D, rp_stream_t stream) {
    RP_REQUIRE(M >= 0 && D >= 1 && M < ((int64_t)1 << 33), "l2norm_bwd: need M >= 0 and D >= 1");
    RP_REQUIRE(x && dy && dx, "l2norm_bwd: null pointer");
    if (M == 0) return RP_OK;
    hipLaunchKernelGGL(sg_l2norm_bwd_kernel, dim3((unsigned)rp_cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, M, D);
    RP_LAUNCH_CHECK("l2norm_bwd");
    return RP_OK;
}

extern "C" int rp_ggnn_geometry(int *max_d, int *max_l, int *rows_per_workgroup, int *lds_bytes) {
    RP_REQUIRE(max_d && max_l && rows_per_workgroup && lds_bytes, "ggnn_geometry: null pointer");
    *max_d = SG_MAX_D, *max_l = SG_MAX_L, *rows_per_workgroup = 64, *lds_bytes = (int)SG_LDS_MAX;
    return RP_OK;
}

extern "C" int rp_ggnn_fits(int L, int D) {
    if (!gg_dims_ok(L, D)) return 0;
    GgArgs a;
    gg_shape(1, L, D, &a);
    return gg_lds_bytes(a) <= SG_LDS_MAX ? 1 : 0;
}

extern "C" int rp_ggnn_cell_workspace_bytes(int64_t B, int L, int D, int backward, size_t *bytes) {
    RP_REQUIRE(bytes, "ggnn_cell_workspace_bytes: null pointer");
    GG_CHECK_DIMS("ggnn_cell_workspace_bytes");
    GgArgs a;
    gg_shape(B, L, D, &a);
    GgWs ws;
    const int rc = gg_ws(a, backward != 0, &ws);
    if (rc != RP_OK) return rc;
    *bytes = ws.total;
    return RP_OK;
}

extern "C" int rp_ggnn_cell_fwd(const float *H, const int32_t *alias, int64_t B, int L, int D, const float *const *params,
                                float *Hout, float *seq_hidden, float *ht, void *workspace, size_t workspace_bytes,
                                rp_stream_t stream) {
    GG_CHECK_DIMS("ggnn_cell_fwd");
    RP_REQUIRE(H && alias && params && workspace && (Hout || seq_hidden || ht), "ggnn_cell_fwd: null pointer");
    GgArgs a;
    gg_shape(B, L, D, &a);
    const size_t lds = gg_lds_bytes(a);
    RP_REQUIRE(lds <= SG_LDS_MAX, "ggnn_cell_fwd: the tile needs %zu bytes of LDS, over %zu", lds, SG_LDS_MAX);
    GgWs ws;
    int rc = gg_ws(a, false, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "ggnn_cell_fwd: workspace too small or misaligned");
    rc = gg_bind(&a, params, workspace, ws, false, "ggnn_cell_fwd");
    if (rc != RP_OK) return rc;
    if (B == 0) return RP_OK;
    a.H = H, a.alias = alias, a.Hout = Hout, a.seq = seq_hidden, a.ht = ht;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gg_pack_kernel, dim3(64), dim3(256), 0, s, a, 0);
    RP_LAUNCH_CHECK("ggnn_cell_fwd (weights)");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gg_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(gg_fwd_kernel, dim3((unsigned)a.nwg), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("ggnn_cell_fwd");
    return RP_OK;
}

extern "C" int rp_ggnn_cell_bwd(const float *H, const int32_t *alias, const float *dHout, const float *dseq_hidden,
                                const float *dht, int64_t B, int L, int D, const float *const *params, float *dH,
                                float *const *grads, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    GG_CHECK_DIMS("ggnn_cell_bwd");
    RP_REQUIRE(H && alias && params && dH && grads && workspace, "ggnn_cell_bwd: null pointer");
    for (int q = 0; q < 8; ++q) RP_REQUIRE(grads[q], "ggnn_cell_bwd: null gradient");
    GgArgs a;
    gg_shape(B, L, D, &a);
    const size_t lds = gg_lds_bytes(a);
    RP_REQUIRE(lds <= SG_LDS_MAX, "ggnn_cell_bwd: the tile needs %zu bytes of LDS, over %zu", lds, SG_LDS_MAX);
    GgWs ws;
    int rc = gg_ws(a, true, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "ggnn_cell_bwd: workspace too small or misaligned");
    rc = gg_bind(&a, params, workspace, ws, true, "ggnn_cell_bwd");
    if (rc != RP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        for (int q = 0; q < 4; ++q) {
            const size_t nw = (size_t)(q < 2 ? D : 3 * D) * (q == 2 ? 2 * D : D), nb = q < 2 ? D : 3 * D;
            (void)hipMemsetAsync(grads[2 * q], 0, 4 * nw, s);
            (void)hipMemsetAsync(grads[2 * q + 1], 0, 4 * nb, s);
        }
        return RP_OK;
    }
    a.H = H, a.alias = alias, a.dHout = dHout, a.dseq = dseq_hidden, a.dht = dht, a.dH = dH;
    hipLaunchKernelGGL(gg_pack_kernel, dim3(64), dim3(256), 0, s, a, 1);
    RP_LAUNCH_CHECK("ggnn_cell_bwd (weights)");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gg_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(gg_bwd_kernel, dim3((unsigned)a.nwg), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("ggnn_cell_bwd");
    char *base = static_cast<char *>(workspace);
    const int64_t M = B * L;
    const float *dy[4] = {a.dP[0], a.dP[1], a.dGI, a.dGH}, *x[4] = {H, H, a.AGG, H};
    const int64_t lddy[4] = {D, D, a.s3, a.s3}, ldx[4] = {D, D, 2 * D, D};
    const int N[4] = {D, D, 3 * D, 3 * D}, K[4] = {D, D, 2 * D, D};
    for (int q = 0; q < 4; ++q) {
        rc = rp_linear_wgrad(dy[q], lddy[q], x[q], ldx[q], grads[2 * q], K[q], grads[2 * q + 1], M, N[q], K[q], 0, base + ws.wgrad,
                             ws.wgrad_bytes, stream);
        if (rc != RP_OK) return rc;
    }
    return RP_OK;
}
