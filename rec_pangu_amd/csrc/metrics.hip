// Epoch metrics on the device, gfx950: binary ROC-AUC as an exact rational and the float64 log-loss sum, from float32
// predictions and labels [n] (what rec_pangu/model_pipeline.py hands to sklearn after a .cpu() of every prediction).
//
//   AUC = 2U / (2 P N),   2U = sum over positives i of (#negatives with pred < pred_i + #negatives with pred <= pred_i)
//
// 2U, P and N are integers (2U <= 2 P N < 2^61 for n < 2^31): whatever the launch geometry, the result is the same three
// numbers, and the host's one division rounds once.  Launches (T = ceil(n / 4096) tiles, one workgroup of 4 waves per tile):
//   metrics_key_kernel        pred, label -> the order-preserving int32 key of every prediction; per tile the counts of
//                             label == 1 / label == 0 / unsupported elements and the float64 sum of the log-loss terms
//   rp_sort_pairs_i32         (key, position) by signed key, stable (sort.hip: 4 digit passes of 3 launches)
//   metrics_tile_sums_kernel  sorted order: label class of every element (fetched through the sorted position, kept as one
//                             byte) ; per tile the number of negatives and of tie-group starts (key != the key before it)
//   metrics_tile_scan_kernel  exclusive scan of both per-tile columns (one workgroup)
//   metrics_group_neg_kernel  Nc[g] = negatives before tie group g, written by the element that starts g; Nc[G] = N
//   metrics_rank_kernel       every positive adds Nc[g] + Nc[g + 1] of its group g -> one int64 partial per tile
//   metrics_finish_kernel     the partials, in a fixed order -> rp_binary_metrics_result (one workgroup)
// A tie group is found per element (a flag and two scans), never walked: one group over the whole array costs what n
// distinct values cost.  Inside a tile the two scans are ballots: both flags are one bit, so a lane's exclusive prefix
// over the 64 elements of a round is a popcount of the ballot below it and the round's total a popcount of all of it; a
// wave walks its 1024 consecutive elements in 16 such rounds and the four waves meet once in LDS.  No atomics anywhere:
// every sum has one order, so two calls give the same bits.  Every launch streams 4-byte elements once (bytes per launch:
// DESIGN 16); the label fetch through the sorted positions is the one random access and is done once.
#include "common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / RP_WAVE;          // 4
constexpr int MT_ROUNDS = 16;                           // elements per thread
constexpr int MT_WAVE_SPAN = MT_ROUNDS * RP_WAVE;       // 1024 consecutive elements per wave
constexpr int MT_TILE = MT_THREADS * MT_ROUNDS;         // 4096 elements per workgroup
constexpr int MT_FIN_THREADS = 1024;
constexpr int MT_FIN_WAVES = MT_FIN_THREADS / RP_WAVE;  // 16

constexpr unsigned char MT_NEG = 0, MT_POS = 1, MT_OTHER = 2;  // label == 0 / label == 1 / anything else

__device__ __forceinline__ int mt_popc(uint64_t m) { return __builtin_popcountll(m); }

// ---- key pass -----------------------------------------------------------------------------------------------------------
// thread t of tile b takes elements b * 4096 + r * 256 + t, r ascending; the float64 terms are summed per thread in that
// order, then across the wave (xor butterfly: every lane forms the same sums), then wave 0..3 in order
__global__ __launch_bounds__(MT_THREADS) void metrics_key_kernel(const float *__restrict__ pred, const float *__restrict__ label,
                                                                 int64_t n, double eps, int want_ll, int32_t *__restrict__ keys,
                                                                 double *__restrict__ part_ll, int32_t *__restrict__ part_p,
                                                                 int32_t *__restrict__ part_n, int32_t *__restrict__ part_u) {
    __shared__ double shd[MT_WAVES];
    __shared__ int32_t shc[MT_WAVES][3];
    const int tid = threadIdx.x, lane = tid & (RP_WAVE - 1), w = tid / RP_WAVE;
    const int64_t base = (int64_t)blockIdx.x * MT_TILE;
    const double hi = 1.0 - eps;
    double acc = 0.0;
    int32_t cp = 0, cn = 0, cu = 0;
#pragma unroll 4
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = base + r * MT_THREADS + tid;
        if (i < n) {
            const float p = pred[i], y = label[i];
            if (keys != nullptr) {
                int32_t k = __float_as_int(p + 0.0f);  // -0.0 + 0.0 = +0.0: one key for both zeros
                if (k < 0) k ^= 0x7FFFFFFF;            // signed integer order == float order
                keys[i] = k;
            }
            const bool one = y == 1.0f, zero = y == 0.0f;
            const bool finite = (__float_as_uint(p) & 0x7F800000u) != 0x7F800000u;
            cp += one;
            cn += zero;
            cu += !(finite && (one || zero));
            if (want_ll) {
                const double q = fmin(fmax((double)p, eps), hi);
                acc -= log(one ? q : 1.0 - q);
            }
        }
    }
#pragma unroll
    for (int o = RP_WAVE / 2; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, RP_WAVE);
        cp += __shfl_xor(cp, o, RP_WAVE);
        cn += __shfl_xor(cn, o, RP_WAVE);
        cu += __shfl_xor(cu, o, RP_WAVE);
    }
    if (lane == 0) {
        shd[w] = acc;
        shc[w][0] = cp;
        shc[w][1] = cn;
        shc[w][2] = cu;
    }
    __syncthreads();
    if (tid == 0) {
        part_ll[blockIdx.x] = (shd[0] + shd[1]) + (shd[2] + shd[3]);
        part_p[blockIdx.x] = shc[0][0] + shc[1][0] + shc[2][0] + shc[3][0];
        part_n[blockIdx.x] = shc[0][1] + shc[1][1] + shc[2][1] + shc[3][1];
        part_u[blockIdx.x] = shc[0][2] + shc[1][2] + shc[2][2] + shc[3][2];
    }
}

// ---- sorted order: the wave's 16 rounds over its 1024 consecutive elements ------------------------------------------------
// bg[r] = ballot of "element (r, lane) starts a tie group": it is element 0, or its key differs from the key before it.
// The key before lane 0's comes from lane 63 of the round before (from memory in round 0).
__device__ __forceinline__ void mt_group_ballots(const int32_t *__restrict__ keys, int64_t first, int64_t n,
                                                 uint64_t (&bg)[MT_ROUNDS]) {
    const int lane = threadIdx.x & (RP_WAVE - 1);
    int32_t carry = (lane == 0 && first > 0 && first < n) ? keys[first - 1] : 0;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = first + r * RP_WAVE + lane;
        const bool valid = i < n;
        const int32_t k = valid ? keys[i] : 0;
        int32_t prev = __shfl_up(k, 1, RP_WAVE);
        if (lane == 0) prev = carry;
        bg[r] = __builtin_amdgcn_ballot_w64(valid && (i == 0 || k != prev));
        carry = __shfl(k, RP_WAVE - 1, RP_WAVE);
    }
}

__global__ __launch_bounds__(MT_THREADS) void metrics_tile_sums_kernel(const int32_t *__restrict__ skeys,
                                                                       const int32_t *__restrict__ spos,
                                                                       const float *__restrict__ label, int64_t n,
                                                                       unsigned char *__restrict__ cls,
                                                                       int32_t *__restrict__ tile_neg,
                                                                       int32_t *__restrict__ tile_grp) {
    __shared__ int32_t sh[MT_WAVES][2];
    const int tid = threadIdx.x, lane = tid & (RP_WAVE - 1), w = tid / RP_WAVE;
    const int64_t first = (int64_t)blockIdx.x * MT_TILE + (int64_t)w * MT_WAVE_SPAN;
    uint64_t bg[MT_ROUNDS];
    mt_group_ballots(skeys, first, n, bg);
    int32_t cn = 0, cg = 0;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = first + r * RP_WAVE + lane;
        unsigned char c = MT_OTHER;
        if (i < n) {
            const float y = label[spos[i]];  // spos is a permutation of [0, n): the sort's positions
            c = y == 0.0f ? MT_NEG : (y == 1.0f ? MT_POS : MT_OTHER);
            cls[i] = c;
        }
        cn += mt_popc(__builtin_amdgcn_ballot_w64(c == MT_NEG));
        cg += mt_popc(bg[r]);
    }
    if (lane == 0) {
        sh[w][0] = cn;
        sh[w][1] = cg;
    }
    __syncthreads();
    if (tid == 0) {
        tile_neg[blockIdx.x] = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        tile_grp[blockIdx.x] = sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1];
    }
}

// one workgroup of 16 waves: a[t], b[t] -> their exclusive prefixes over the tiles, in place (sums <= n < 2^31)
__global__ __launch_bounds__(MT_FIN_THREADS) void metrics_tile_scan_kernel(int32_t *__restrict__ a, int32_t *__restrict__ b,
                                                                           int64_t ntiles) {
    __shared__ int32_t ws[2][MT_FIN_WAVES];
    const int tid = threadIdx.x, lane = tid & (RP_WAVE - 1), w = tid / RP_WAVE;
    int32_t carry_a = 0, carry_b = 0;
    for (int64_t t0 = 0; t0 < ntiles; t0 += MT_FIN_THREADS) {
        const int64_t t = t0 + tid;
        const int32_t va = t < ntiles ? a[t] : 0, vb = t < ntiles ? b[t] : 0;
        int32_t sa = va, sb = vb;
#pragma unroll
        for (int o = 1; o < RP_WAVE; o <<= 1) {
            const int32_t ua = __shfl_up(sa, o, RP_WAVE), ub = __shfl_up(sb, o, RP_WAVE);
            if (lane >= o) {
                sa += ua;
                sb += ub;
            }
        }
        if (lane == RP_WAVE - 1) {
            ws[0][w] = sa;
            ws[1][w] = sb;
        }
        __syncthreads();
        int32_t before_a = 0, before_b = 0, tot_a = 0, tot_b = 0;
#pragma unroll
        for (int x = 0; x < MT_FIN_WAVES; ++x) {
            const int32_t xa = ws[0][x], xb = ws[1][x];
            if (x < w) {
                before_a += xa;
                before_b += xb;
            }
            tot_a += xa;
            tot_b += xb;
        }
        if (t < ntiles) {
            a[t] = carry_a + before_a + sa - va;
            b[t] = carry_b + before_b + sb - vb;
        }
        carry_a += tot_a;
        carry_b += tot_b;
        __syncthreads();  // ws is rewritten by the next chunk
    }
}

// The wave's offsets inside the sorted order: (negatives, group starts) before its first element = the tile's scanned
// sums + the totals of the waves before it in the tile.
__device__ __forceinline__ void mt_wave_offsets(int32_t (*sh)[2], int32_t cn, int32_t cg, int32_t tile_n, int32_t tile_g,
                                                int32_t &on, int32_t &og) {
    const int lane = threadIdx.x & (RP_WAVE - 1), w = threadIdx.x / RP_WAVE;
    if (lane == 0) {
        sh[w][0] = cn;
        sh[w][1] = cg;
    }
    __syncthreads();
    on = tile_n;
    og = tile_g;
    for (int x = 0; x < w; ++x) {
        on += sh[x][0];
        og += sh[x][1];
    }
}

// nc has n + 1 entries; entry g <= (number of groups) <= n is written exactly once
__global__ __launch_bounds__(MT_THREADS) void metrics_group_neg_kernel(const int32_t *__restrict__ skeys,
                                                                       const unsigned char *__restrict__ cls, int64_t n,
                                                                       const int32_t *__restrict__ tile_neg,
                                                                       const int32_t *__restrict__ tile_grp,
                                                                       int32_t *__restrict__ nc) {
    __shared__ int32_t sh[MT_WAVES][2];
    const int lane = threadIdx.x & (RP_WAVE - 1), w = threadIdx.x / RP_WAVE;
    const int64_t first = (int64_t)blockIdx.x * MT_TILE + (int64_t)w * MT_WAVE_SPAN;
    uint64_t bg[MT_ROUNDS], bn[MT_ROUNDS];
    mt_group_ballots(skeys, first, n, bg);
    int32_t cn = 0, cg = 0;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = first + r * RP_WAVE + lane;
        const unsigned char c = i < n ? cls[i] : MT_OTHER;
        bn[r] = __builtin_amdgcn_ballot_w64(c == MT_NEG);
        cn += mt_popc(bn[r]);
        cg += mt_popc(bg[r]);
    }
    int32_t on, og;
    mt_wave_offsets(sh, cn, cg, tile_neg[blockIdx.x], tile_grp[blockIdx.x], on, og);
    const uint64_t lower = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = first + r * RP_WAVE + lane;
        if (i < n) {
            const int32_t neg_before = on + mt_popc(bn[r] & lower);   // negatives at sorted places < i
            const int32_t starts_before = og + mt_popc(bg[r] & lower);  // group starts at sorted places < i
            const int32_t is_start = (int32_t)((bg[r] >> lane) & 1ull), is_neg = (int32_t)((bn[r] >> lane) & 1ull);
            if (is_start) nc[starts_before] = neg_before;  // i opens group number starts_before
            if (i == n - 1) nc[starts_before + is_start] = neg_before + is_neg;  // one past the last group: all negatives
        }
        on += mt_popc(bn[r]);
        og += mt_popc(bg[r]);
    }
}

__global__ __launch_bounds__(MT_THREADS) void metrics_rank_kernel(const int32_t *__restrict__ skeys,
                                                                  const unsigned char *__restrict__ cls, int64_t n,
                                                                  const int32_t *__restrict__ tile_grp,
                                                                  const int32_t *__restrict__ nc,
                                                                  int64_t *__restrict__ part_2u) {
    __shared__ int32_t sh[MT_WAVES][2];
    __shared__ int64_t shs[MT_WAVES];
    const int lane = threadIdx.x & (RP_WAVE - 1), w = threadIdx.x / RP_WAVE;
    const int64_t first = (int64_t)blockIdx.x * MT_TILE + (int64_t)w * MT_WAVE_SPAN;
    uint64_t bg[MT_ROUNDS];
    mt_group_ballots(skeys, first, n, bg);
    int32_t cg = 0;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) cg += mt_popc(bg[r]);
    int32_t on, og;
    mt_wave_offsets(sh, 0, cg, 0, tile_grp[blockIdx.x], on, og);
    (void)on;
    const uint64_t lower = (1ull << lane) - 1ull;
    int64_t acc = 0;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int64_t i = first + r * RP_WAVE + lane;
        if (i < n && cls[i] == MT_POS) {
            // the element's group: the starts at sorted places <= i, minus one (element 0 is a start, so g >= 0; g + 1 <= n)
            const int32_t g = og + mt_popc(bg[r] & lower) + (int32_t)((bg[r] >> lane) & 1ull) - 1;
            acc += (int64_t)nc[g] + (int64_t)nc[g + 1];
        }
        og += mt_popc(bg[r]);
    }
#pragma unroll
    for (int o = RP_WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, RP_WAVE);
    if (lane == 0) shs[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part_2u[blockIdx.x] = (shs[0] + shs[1]) + (shs[2] + shs[3]);
}

// one workgroup: thread t sums partials t, t + 1024, ... in ascending order, then the wave butterfly, then waves 0..15 in order
__global__ __launch_bounds__(MT_FIN_THREADS) void metrics_finish_kernel(const double *__restrict__ part_ll,
                                                                        const int32_t *__restrict__ part_p,
                                                                        const int32_t *__restrict__ part_n,
                                                                        const int32_t *__restrict__ part_u,
                                                                        const int64_t *__restrict__ part_2u, int64_t ntiles,
                                                                        rp_binary_metrics_result *__restrict__ result) {
    __shared__ double shd[MT_FIN_WAVES];
    __shared__ int64_t shi[MT_FIN_WAVES][4];
    const int tid = threadIdx.x, lane = tid & (RP_WAVE - 1), w = tid / RP_WAVE;
    double ll = 0.0;
    int64_t p = 0, ng = 0, u = 0, two_u = 0;
    for (int64_t t = tid; t < ntiles; t += MT_FIN_THREADS) {
        ll += part_ll[t];
        p += part_p[t];
        ng += part_n[t];
        u += part_u[t];
        if (part_2u != nullptr) two_u += part_2u[t];
    }
#pragma unroll
    for (int o = RP_WAVE / 2; o > 0; o >>= 1) {
        ll += __shfl_xor(ll, o, RP_WAVE);
        p += __shfl_xor(p, o, RP_WAVE);
        ng += __shfl_xor(ng, o, RP_WAVE);
        u += __shfl_xor(u, o, RP_WAVE);
        two_u += __shfl_xor(two_u, o, RP_WAVE);
    }
    if (lane == 0) {
        shd[w] = ll;
        shi[w][0] = p;
        shi[w][1] = ng;
        shi[w][2] = u;
        shi[w][3] = two_u;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int64_t c[4] = {0, 0, 0, 0};
        for (int x = 0; x < MT_FIN_WAVES; ++x) {
            s += shd[x];
            for (int j = 0; j < 4; ++j) c[j] += shi[x][j];
        }
        result->two_u = c[3];
        result->P = c[0];
        result->N = c[1];
        result->unsupported = c[2];
        result->logloss_sum = s;
    }
}

size_t mt_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [keys n + 1 | sorted keys n | sorted positions n | the sort's workspace | class bytes n | tile columns and partials]
// The unsorted keys are dead once the sort has read them: the same n + 1 ints then hold Nc.
struct MetricsPlan {
    int64_t ntiles;
    size_t sort_bytes;
    size_t off_skeys, off_spos, off_sort, off_cls, off_tneg, off_tgrp, off_pll, off_pp, off_pn, off_pu, off_p2u, bytes;
};

int metrics_plan(int64_t n, MetricsPlan *p) {
    p->ntiles = rp_cdiv(n, MT_TILE);
    const int rc = rp_sort_workspace_bytes(n, &p->sort_bytes);
    if (rc != RP_OK) return rc;
    const size_t T = (size_t)p->ntiles;
    size_t off = mt_align256(((size_t)n + 1) * sizeof(int32_t));
    p->off_skeys = off, off += mt_align256((size_t)n * sizeof(int32_t));
    p->off_spos = off, off += mt_align256((size_t)n * sizeof(int32_t));
    p->off_sort = off, off += mt_align256(p->sort_bytes);
    p->off_cls = off, off += mt_align256((size_t)n);
    p->off_tneg = off, off += mt_align256(T * sizeof(int32_t));
    p->off_tgrp = off, off += mt_align256(T * sizeof(int32_t));
    p->off_pll = off, off += mt_align256(T * sizeof(double));
    p->off_pp = off, off += mt_align256(T * sizeof(int32_t));
    p->off_pn = off, off += mt_align256(T * sizeof(int32_t));
    p->off_pu = off, off += mt_align256(T * sizeof(int32_t));
    p->off_p2u = off, off += mt_align256(T * sizeof(int64_t));
    p->bytes = off;
    return RP_OK;
}

bool mt_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int rp_metrics_workspace_bytes(int64_t n, size_t *bytes) {
    RP_REQUIRE(bytes != nullptr, "metrics_workspace_bytes: null pointer");
    RP_REQUIRE(n >= 1 && n < INT32_MAX, "metrics_workspace_bytes: n = %lld outside [1, 2^31 - 1)", (long long)n);
    MetricsPlan p;
    const int rc = metrics_plan(n, &p);
    if (rc != RP_OK) return rc;
    *bytes = p.bytes + 256;
    return RP_OK;
}

extern "C" int rp_binary_metrics(void *workspace, size_t workspace_bytes, const float *pred, const float *label, int64_t n,
                                 double eps, int flags, rp_binary_metrics_result *result, rp_stream_t stream) {
    RP_REQUIRE(workspace && pred && label && result, "binary_metrics: null pointer");
    RP_REQUIRE(n >= 1 && n < INT32_MAX, "binary_metrics: n = %lld outside [1, 2^31 - 1)", (long long)n);
    RP_REQUIRE((flags & (RP_METRIC_AUC | RP_METRIC_LOGLOSS)) != 0 && (flags & ~(RP_METRIC_AUC | RP_METRIC_LOGLOSS | RP_METRICS_STAGE_ALL)) == 0,
               "binary_metrics: flags 0x%x name no metric or an unknown bit", flags);
    RP_REQUIRE(eps >= 0.0 && eps < 0.5, "binary_metrics: eps outside [0, 0.5)");
    MetricsPlan p;
    int rc = metrics_plan(n, &p);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= p.bytes + 256, "binary_metrics: workspace %zu < %zu bytes", workspace_bytes, p.bytes + 256);
    const size_t col = (size_t)n * sizeof(float);
    RP_REQUIRE(!mt_overlap(pred, col, label, col) && !mt_overlap(pred, col, result, sizeof(*result)) &&
                   !mt_overlap(label, col, result, sizeof(*result)) && !mt_overlap(workspace, workspace_bytes, pred, col) &&
                   !mt_overlap(workspace, workspace_bytes, label, col) &&
                   !mt_overlap(workspace, workspace_bytes, result, sizeof(*result)),
               "binary_metrics: buffers alias");
    RP_REQUIRE((reinterpret_cast<uintptr_t>(result) & 7u) == 0, "binary_metrics: result is not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int32_t *keys = reinterpret_cast<int32_t *>(base), *nc = keys;
    int32_t *skeys = reinterpret_cast<int32_t *>(base + p.off_skeys), *spos = reinterpret_cast<int32_t *>(base + p.off_spos);
    unsigned char *cls = reinterpret_cast<unsigned char *>(base + p.off_cls);
    int32_t *tile_neg = reinterpret_cast<int32_t *>(base + p.off_tneg), *tile_grp = reinterpret_cast<int32_t *>(base + p.off_tgrp);
    double *part_ll = reinterpret_cast<double *>(base + p.off_pll);
    int32_t *part_p = reinterpret_cast<int32_t *>(base + p.off_pp), *part_n = reinterpret_cast<int32_t *>(base + p.off_pn);
    int32_t *part_u = reinterpret_cast<int32_t *>(base + p.off_pu);
    int64_t *part_2u = reinterpret_cast<int64_t *>(base + p.off_p2u);
    const bool auc = (flags & RP_METRIC_AUC) != 0;
    // a measurement may issue the stages one call at a time over the same workspace (profiles/microbench/metrics_epoch.py)
    const int stages = (flags & RP_METRICS_STAGE_ALL) ? (flags & RP_METRICS_STAGE_ALL) : RP_METRICS_STAGE_ALL;
    const dim3 tiles((unsigned)p.ntiles), block(MT_THREADS);

    if (stages & RP_METRICS_STAGE_KEY) {
        hipLaunchKernelGGL(metrics_key_kernel, tiles, block, 0, s, pred, label, n, eps, (flags & RP_METRIC_LOGLOSS) ? 1 : 0,
                           auc ? keys : (int32_t *)nullptr, part_ll, part_p, part_n, part_u);
        RP_LAUNCH_CHECK("metrics_key");
    }
    if (auc) {
        if (stages & RP_METRICS_STAGE_SORT) {
            rc = rp_sort_pairs_i32(base + p.off_sort, p.sort_bytes, keys, skeys, spos, n, 32, stream);
            if (rc != RP_OK) return rc;
        }
        if (stages & RP_METRICS_STAGE_TILE_SUMS) {
            hipLaunchKernelGGL(metrics_tile_sums_kernel, tiles, block, 0, s, skeys, spos, label, n, cls, tile_neg, tile_grp);
            RP_LAUNCH_CHECK("metrics_tile_sums");
        }
        if (stages & RP_METRICS_STAGE_TILE_SCAN) {
            hipLaunchKernelGGL(metrics_tile_scan_kernel, dim3(1), dim3(MT_FIN_THREADS), 0, s, tile_neg, tile_grp, p.ntiles);
            RP_LAUNCH_CHECK("metrics_tile_scan");
        }
        if (stages & RP_METRICS_STAGE_GROUP_NEG) {
            hipLaunchKernelGGL(metrics_group_neg_kernel, tiles, block, 0, s, skeys, cls, n, tile_neg, tile_grp, nc);
            RP_LAUNCH_CHECK("metrics_group_neg");
        }
        if (stages & RP_METRICS_STAGE_RANK) {
            hipLaunchKernelGGL(metrics_rank_kernel, tiles, block, 0, s, skeys, cls, n, tile_grp, nc, part_2u);
            RP_LAUNCH_CHECK("metrics_rank");
        }
    }
    if (stages & RP_METRICS_STAGE_FINISH) {
        hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MT_FIN_THREADS), 0, s, part_ll, part_p, part_n, part_u,
                           auc ? part_2u : (int64_t *)nullptr, p.ntiles, result);
        RP_LAUNCH_CHECK("metrics_finish");
    }
    return RP_OK;
}
