// The key-padding (non-causal) mode of the sequence attention core, gfx950: the attention of the reference's BERT4RecEncoder
// (rec_pangu/models/layers/sequence.py:150-186, MultiHeadAttention.scaled_dot_product_attention under
// masked_fill(mask == 0, -inf)).  Same layouts and limits as seq_attn.hip (q, k, v are column blocks of projected rows, ctx is
// head-interleaved, L <= 128, dh <= 64), and the same two modes.
//
// Per (b, head):  ctx[i, :] = sum_{j content} softmax_j(q_i . k_j / sqrt(dh)) v_j  for EVERY query row i, padded ones included.
// A masked key has probability exactly 0: it is skipped, not given an additive score, so its dK and dV rows are exactly 0.
// A sample without a content key gets zero context rows and passes zero gradients (the reference: softmax of a row of -inf
// is NaN, which it replaces by 0).  No dropout: the reference's layer has none on the probabilities.
//
// (a) Full mode: a workgroup per (b, head), a thread per query row, K and V tiles in LDS, an online softmax over the content
//     keys; saved: lse[b, head, i] = max + log(sum) (0 for a sample without content).  Backward, one launch: phase A
//     (thread = query row) forms delta_i = sum_j p_ij (dctx_i . v_j) from the recomputed probabilities, then dQ_i; phase B
//     (thread = key row) dK_j and dV_j over all L queries; fixed order, no atomics.  delta comes from the same p and the
//     same dot products ds_ij = p_ij (dctx_i . v_j - delta_i) uses, not from dctx . ctx: a sample with ONE content key
//     (p = 1) then has ds = 0 exactly, as in exact arithmetic, instead of the rounding of two differently ordered sums
//     added up over L queries.  ctx is not an input of the backward.
// (b) Last-row mode: qpos[b] selects one query per sample; a wave per (b, head), lane = key (two per lane).  qpos[b] < 0: zero
//     row, zero gradients.
#include "common.h"
#include "seq_attn_dev.h"

#include <math.h>

namespace {

// grid B heads, block 64 ceil(L / 64); dynamic LDS: ks [L][DH], vs [L][DH], km [L] (1 = content)
template <int DH>
__global__ __launch_bounds__(128) void seq_attn_kp_fwd_kernel(const float *__restrict__ q, int64_t ldq, const float *__restrict__ kv,
                                                              int64_t ldkv, const float *__restrict__ mask, int L, int heads,
                                                              int dh, float sq, float *__restrict__ ctx, float *__restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    float *ks = sa_lds, *vs = ks + L * DH, *km = vs + L * DH;
    const int h = blockIdx.x % heads, i = threadIdx.x, D = heads * dh;
    const int64_t b = blockIdx.x / heads, row0 = b * L;
    sa_stage<DH>(kv, ldkv, row0, h * dh, L, dh, ks);
    sa_stage<DH>(kv, ldkv, row0, D + h * dh, L, dh, vs);
    for (int j = threadIdx.x; j < L; j += blockDim.x) km[j] = mask[row0 + j] != 0.f ? 1.f : 0.f;
    __syncthreads();
    if (i >= L) return;  // (behind the only barrier)
    float qr[DH], acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) qr[d] = d < dh ? q[(row0 + i) * ldq + h * dh + d] : 0.f, acc[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < L; ++j) {
        if (km[j] == 0.f) continue;
        const float s = sa_dot<DH>(qr, ks + j * DH) / sq;
        const float mn = fmaxf(m, s), a = expf(m - mn), e = expf(s - mn);  // (exp(-inf - mn) = 0 at the first key)
        l = l * a + e;
        m = mn;
        const float *vj = vs + j * DH;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(vj + d);
            acc[d] = acc[d] * a + e * t[0];
            acc[d + 1] = acc[d + 1] * a + e * t[1];
            acc[d + 2] = acc[d + 2] * a + e * t[2];
            acc[d + 3] = acc[d + 3] * a + e * t[3];
        }
    }
    const bool any = l > 0.f;  // (the maximum's own term is 1)
    float *o = ctx + (row0 + i) * D + h * dh;
#pragma unroll
    for (int d = 0; d < DH; ++d)
        if (d < dh) o[d] = any ? acc[d] / l : 0.f;
    lse[(int64_t)blockIdx.x * L + i] = any ? m + logf(l) : 0.f;
}

// grid B heads, block 64 ceil(L / 64); dynamic LDS: qs, ks, vs, gs [L][DH] each, km, ls, dl [L] each
template <int DH>
__global__ __launch_bounds__(128) void seq_attn_kp_bwd_kernel(const float *__restrict__ q, int64_t ldq, const float *__restrict__ kv,
                                                              int64_t ldkv, const float *__restrict__ mask,
                                                              const float *__restrict__ dctx,
                                                              const float *__restrict__ lse, int L, int heads, int dh, float sq,
                                                              float *__restrict__ dq, int64_t lddq, float *__restrict__ dkv,
                                                              int64_t lddkv) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    float *qs = sa_lds, *ks = qs + L * DH, *vs = ks + L * DH, *gs = vs + L * DH, *km = gs + L * DH, *ls = km + L, *dl = ls + L;
    const int h = blockIdx.x % heads, t = threadIdx.x, D = heads * dh;
    const int64_t b = blockIdx.x / heads, row0 = b * L, hrow0 = (int64_t)blockIdx.x * L;
    sa_stage<DH>(q, ldq, row0, h * dh, L, dh, qs);
    sa_stage<DH>(kv, ldkv, row0, h * dh, L, dh, ks);
    sa_stage<DH>(kv, ldkv, row0, D + h * dh, L, dh, vs);
    sa_stage<DH>(dctx, D, row0, h * dh, L, dh, gs);
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        km[j] = mask[row0 + j] != 0.f ? 1.f : 0.f;
        ls[j] = lse[hrow0 + j];
    }
    __syncthreads();
    if (t < L) {  // phase A: thread = query row i; delta_i, then dQ_i = sum_{j content} ds_ij k_j / sqrt(dh)
        const int i = t;
        float qr[DH], gr[DH], dqr[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) qr[d] = qs[i * DH + d], gr[d] = gs[i * DH + d], dqr[d] = 0.f;
        const float li = ls[i];
        float di = 0.f;
        for (int j = 0; j < L; ++j) {
            if (km[j] == 0.f) continue;
            di += expf(sa_dot<DH>(qr, ks + j * DH) / sq - li) * sa_dot<DH>(gr, vs + j * DH);
        }
        dl[i] = di;
        for (int j = 0; j < L; ++j) {
            if (km[j] == 0.f) continue;
            const float s = sa_dot<DH>(qr, ks + j * DH) / sq;
            const float p = expf(s - li);
            const float ds = p * (sa_dot<DH>(gr, vs + j * DH) - di);
            const float *kj = ks + j * DH;
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const f32x4 k4 = *reinterpret_cast<const f32x4 *>(kj + d);
                dqr[d] += ds * k4[0];
                dqr[d + 1] += ds * k4[1];
                dqr[d + 2] += ds * k4[2];
                dqr[d + 3] += ds * k4[3];
            }
        }
        float *o = dq + (row0 + i) * lddq + h * dh;
#pragma unroll
        for (int d = 0; d < DH; ++d)
            if (d < dh) o[d] = dqr[d] / sq;
    }
    __syncthreads();
    if (t < L) {  // phase B: thread = key row j; dK_j = sum_i ds_ij q_i / sqrt(dh), dV_j = sum_i p_ij dctx_i; zero rows for a masked key
        const int j = t;
        float kr[DH], vr[DH], dkr[DH], dvr[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) kr[d] = ks[j * DH + d], vr[d] = vs[j * DH + d], dkr[d] = 0.f, dvr[d] = 0.f;
        if (km[j] != 0.f) {
            for (int i = 0; i < L; ++i) {
                const float s = sa_dot<DH>(kr, qs + i * DH) / sq;
                const float p = expf(s - ls[i]);
                const float ds = p * (sa_dot<DH>(vr, gs + i * DH) - dl[i]);
                const float *qi = qs + i * DH, *gi = gs + i * DH;
#pragma unroll
                for (int d = 0; d < DH; d += 4) {
                    const f32x4 q4 = *reinterpret_cast<const f32x4 *>(qi + d), g4 = *reinterpret_cast<const f32x4 *>(gi + d);
                    dkr[d] += ds * q4[0], dvr[d] += p * g4[0];
                    dkr[d + 1] += ds * q4[1], dvr[d + 1] += p * g4[1];
                    dkr[d + 2] += ds * q4[2], dvr[d + 2] += p * g4[2];
                    dkr[d + 3] += ds * q4[3], dvr[d + 3] += p * g4[3];
                }
            }
        }
        float *ok = dkv + (row0 + j) * lddkv + h * dh, *ov = ok + D;
#pragma unroll
        for (int d = 0; d < DH; ++d)
            if (d < dh) ok[d] = dkr[d] / sq, ov[d] = dvr[d];
    }
}

// grid B heads, block 64
__global__ __launch_bounds__(64) void seq_attn_kp_last_fwd_kernel(const float *__restrict__ q, int64_t ldq, int compact,
                                                                  const float *__restrict__ kv, int64_t ldkv,
                                                                  const float *__restrict__ mask, const int64_t *__restrict__ qpos,
                                                                  int L, int heads, int dh, float sq, float *__restrict__ ctx,
                                                                  float *__restrict__ lse) {
    __shared__ float qv[SA_MAX_DH], pb[SA_MAX_L];
    const int h = blockIdx.x % heads, lane = threadIdx.x, D = heads * dh;
    const int64_t b = blockIdx.x / heads, row0 = b * L;
    const int64_t qp = qpos[b];
    if (qp < 0) {  // (uniform over the workgroup) no history: a zero row
        if (lane < dh) ctx[b * D + h * dh + lane] = 0.f;
        if (lane == 0) lse[blockIdx.x] = 0.f;
        return;
    }
    const int i = qp < L ? (int)qp : L - 1;
    if (lane < dh) qv[lane] = q[(compact ? b : row0 + i) * ldq + h * dh + lane];
    __syncthreads();
    float s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        s[t] = (j < L && mask[row0 + j] != 0.f) ? sa_last_score(qv, kv + (row0 + j) * ldkv + h * dh, dh, sq, 0.f) : -INFINITY;
    }
    const float m = rp_lane_max(fmaxf(s[0], s[1]));
    const bool any = m > -INFINITY;  // (uniform over the wave)
    const float e0 = any ? expf(s[0] - m) : 0.f, e1 = any ? expf(s[1] - m) : 0.f;
    const float l = rp_lane_sum(e0 + e1);
    pb[lane] = e0;
    pb[lane + 64] = e1;
    __syncthreads();
    if (lane < dh) {
        float o = 0.f;
        for (int j = 0; j < L; ++j)
            if (pb[j] != 0.f) o += pb[j] * kv[(row0 + j) * ldkv + D + h * dh + lane];
        ctx[b * D + h * dh + lane] = any ? o / l : 0.f;
    }
    if (lane == 0) lse[blockIdx.x] = any ? m + logf(l) : 0.f;
}

// grid B heads, block 64.  WRITES this head's columns of dK, dV for all L rows, and of dQ: compact: row b of dq [B, .];
// otherwise all L rows of the sample (zeros but for row qpos[b])
__global__ __launch_bounds__(64) void seq_attn_kp_last_bwd_kernel(const float *__restrict__ q, int64_t ldq, int compact,
                                                                  const float *__restrict__ kv, int64_t ldkv,
                                                                  const float *__restrict__ mask, const int64_t *__restrict__ qpos,
                                                                  const float *__restrict__ dctx,
                                                                  const float *__restrict__ lse, int L, int heads, int dh, float sq,
                                                                  float *__restrict__ dq, int64_t lddq, float *__restrict__ dkv,
                                                                  int64_t lddkv) {
    __shared__ float qv[SA_MAX_DH], gv[SA_MAX_DH], dsb[SA_MAX_L];
    const int h = blockIdx.x % heads, lane = threadIdx.x, D = heads * dh;
    const int64_t b = blockIdx.x / heads, row0 = b * L;
    const int64_t qp = qpos[b];
    const int i = qp < 0 ? -1 : (qp < L ? (int)qp : L - 1);
    if (i >= 0 && lane < dh) {
        qv[lane] = q[(compact ? b : row0 + i) * ldq + h * dh + lane];
        gv[lane] = dctx[b * D + h * dh + lane];
    }
    __syncthreads();
    const float li = i >= 0 ? lse[blockIdx.x] : 0.f;
    float pj[2] = {0.f, 0.f}, gvj[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        if (j < L && i >= 0 && mask[row0 + j] != 0.f) {
            const float *krow = kv + (row0 + j) * ldkv + h * dh, *vrow = krow + D;
            pj[t] = expf(sa_last_score(qv, krow, dh, sq, 0.f) - li);
            for (int d = 0; d < dh; ++d) gvj[t] += gv[d] * vrow[d];
        }
    }
    const float delta = rp_lane_sum(pj[0] * gvj[0] + pj[1] * gvj[1]);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        dsb[j] = 0.f;
        if (j >= L) continue;
        float *ok = dkv + (row0 + j) * lddkv + h * dh, *ov = ok + D;
        if (i >= 0 && mask[row0 + j] != 0.f) {
            const float p = pj[t];
            const float ds = p * (gvj[t] - delta);
            for (int d = 0; d < dh; ++d) ok[d] = ds * qv[d] / sq, ov[d] = p * gv[d];
            dsb[j] = ds;
        } else {
            for (int d = 0; d < dh; ++d) ok[d] = 0.f, ov[d] = 0.f;
        }
        if (!compact && j != i) {
            float *oq = dq + (row0 + j) * lddq + h * dh;
            for (int d = 0; d < dh; ++d) oq[d] = 0.f;
        }
    }
    __syncthreads();
    if (lane < dh) {
        float acc = 0.f;
        for (int j = 0; j < L; ++j)
            if (dsb[j] != 0.f) acc += dsb[j] * kv[(row0 + j) * ldkv + h * dh + lane];
        if (compact) dq[b * lddq + h * dh + lane] = acc / sq;
        else if (i >= 0) dq[(row0 + i) * lddq + h * dh + lane] = acc / sq;
    }
}

#define SAK_CHECK(what)                                                                                                     \
    RP_REQUIRE(B >= 0 && B * (int64_t)heads <= (int64_t)INT32_MAX && sa_fits(L, heads, dh),                                 \
               what ": need 0 <= B heads < 2^31, 1 <= L <= %d, 1 <= dh <= %d, heads >= 1 (got B=%lld L=%d heads=%d dh=%d)", \
               SA_MAX_L, SA_MAX_DH, (long long)B, L, heads, dh);                                                           \
    RP_REQUIRE(ldq >= (int64_t)heads * dh && ldkv >= 2 * (int64_t)heads * dh, what ": rows narrower than heads dh / 2 heads dh")

}  // namespace

extern "C" int rp_seq_attn_keypad_fwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                                      const int64_t *qpos, int64_t B, int L, int heads, int dh, float *ctx, float *lse,
                                      rp_stream_t stream) {
    SAK_CHECK("seq_attn_keypad_fwd");
    RP_REQUIRE(q && kv && mask && ctx && lse, "seq_attn_keypad_fwd: null pointer");
    RP_REQUIRE(qpos != nullptr || !q_compact, "seq_attn_keypad_fwd: compact query rows need qpos");
    if (B == 0) return RP_OK;
    const float sq = (float)sqrt((double)dh);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * heads));
    if (qpos != nullptr) {
        hipLaunchKernelGGL(seq_attn_kp_last_fwd_kernel, grid, dim3(64), 0, s, q, ldq, q_compact, kv, ldkv, mask, qpos, L, heads, dh,
                           sq, ctx, lse);
    } else {
        const int DHP = sa_pad_dh(dh);
        const size_t lds = sizeof(float) * ((size_t)2 * L * DHP + L);
        const dim3 block(64 * (unsigned)rp_cdiv(L, SA_ROWS));
#define SAK_FWD(W)                                                                                                                \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(seq_attn_kp_fwd_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                              (int)lds);                                                                                          \
    hipLaunchKernelGGL(seq_attn_kp_fwd_kernel<W>, grid, block, (unsigned)lds, s, q, ldq, kv, ldkv, mask, L, heads, dh, sq, ctx, lse)
        SA_DISPATCH(DHP, SAK_FWD)
#undef SAK_FWD
    }
    RP_LAUNCH_CHECK("seq_attn_keypad_fwd");
    return RP_OK;
}

extern "C" int rp_seq_attn_keypad_bwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                                      const int64_t *qpos, const float *dctx, const float *lse, int64_t B, int L,
                                      int heads, int dh, float *dq, int64_t lddq, float *dkv, int64_t lddkv, rp_stream_t stream) {
    SAK_CHECK("seq_attn_keypad_bwd");
    RP_REQUIRE(q && kv && mask && dctx && lse && dq && dkv, "seq_attn_keypad_bwd: null pointer");
    RP_REQUIRE(qpos != nullptr || !q_compact, "seq_attn_keypad_bwd: compact query rows need qpos");
    RP_REQUIRE(lddq >= (int64_t)heads * dh && lddkv >= 2 * (int64_t)heads * dh, "seq_attn_keypad_bwd: gradient rows too narrow");
    if (B == 0) return RP_OK;
    const float sq = (float)sqrt((double)dh);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * heads));
    if (qpos != nullptr) {
        hipLaunchKernelGGL(seq_attn_kp_last_bwd_kernel, grid, dim3(64), 0, s, q, ldq, q_compact, kv, ldkv, mask, qpos, dctx, lse,
                           L, heads, dh, sq, dq, lddq, dkv, lddkv);
    } else {
        const int DHP = sa_pad_dh(dh);
        const size_t lds = sizeof(float) * ((size_t)4 * L * DHP + 3 * L);
        const dim3 block(64 * (unsigned)rp_cdiv(L, SA_ROWS));
#define SAK_BWD(W)                                                                                                                \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(seq_attn_kp_bwd_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                              (int)lds);                                                                                          \
    hipLaunchKernelGGL(seq_attn_kp_bwd_kernel<W>, grid, block, (unsigned)lds, s, q, ldq, kv, ldkv, mask, dctx, lse, L, heads,  \
                       dh, sq, dq, lddq, dkv, lddkv)
        SA_DISPATCH(DHP, SAK_BWD)
#undef SAK_BWD
    }
    RP_LAUNCH_CHECK("seq_attn_keypad_bwd");
    return RP_OK;
}
