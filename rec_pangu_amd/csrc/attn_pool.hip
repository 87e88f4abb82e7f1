// Two-layer additive attention over a history's rows followed by pooling of those same rows, gfx950 — replaces STAMPLayer's
// attention (rec_pangu/models/layers/sequence.py:131-137: attn_i, attn_e, the masked weights and the weighted sum) and
// MultiInterestSelfAttention.forward (rec_pangu/models/layers/multi_interest.py:37-51) with their autograd:
//
//     S[b, l, k] = sum_h W2[h, k] act((X[b, l, :] . W1)[h] + c[b, h])          act: sigmoid or tanh, c optional
//     A = S valid  (mask)   or   softmax over l of (valid ? S : -1e9)          (softmax)
//     out[b, k, :] = sum_l A[b, l, k] X[b, l, :]
//
// The hidden tensor act(X W1 + c) [B, L, Dh] never exists in memory: not in the forward, not saved for the backward.
//
// ap_fwd_kernel: a workgroup of 256 threads owns TS = floor(64 / L) samples (TS L <= 64 rows, padded to 32); their X tile
//   [Mp][Dp + 4] sits in LDS.  Dh is walked in chunks of 32 columns: a wave takes one row tile and every (4 / row tiles)-th
//   chunk, forms the pre-activation tile on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32) against a zero-padded
//   transposed copy of W1 in the workspace (one small launch per call) — as the TRANSPOSED product, so a lane holds one
//   row of the tile and 16 of the chunk's columns —, applies the activation in registers, multiplies by the chunk's W2 rows
//   and sums over the columns in the lane (one exchange between the wave's halves, a fixed order); a row's scores stay in
//   registers across the wave's chunks and go to the wave's own score slab in LDS, the slabs of a row tile are added in
//   wave order.  Then one thread per (sample, head) normalises over the L positions and the pooled rows are formed from
//   the tile.
//
// ap_bwd_kernel: the same walk recomputes the hidden chunk; dA[l, k] = dout[k, :] . X[l, :], dS through the mask or the
//   softmax (a position with valid = 0 takes none: its score is a constant), dPre = (dS W2^T) act' goes to stacked rows
//   [B L, Dhs] in the workspace, dW2 to a per-workgroup slab (LDS while the workgroup walks its groups of samples, then
//   global; a finishing launch adds the slabs in workgroup order).  dX = A dout + dPre W1^T runs on the matrix core from the
//   workgroup's own stacked rows, dc sums them per sample, dW1 = X^T dPre is one rp_linear_wgrad over the stacked rows.
//   No floating-point atomics: two runs give the same bits.
#include "common.h"

namespace {

constexpr int AP_MAX_D = 128, AP_MAX_DH = 512, AP_MAX_K = 8, AP_MAX_L = 64, AP_SLABS = 1024;
constexpr size_t AP_LDS_MAX = 160 * 1024 - 512;
constexpr float AP_MASKED = -1e9f;

struct ApArgs {
    const float *X, *valid, *W1, *W2, *c;  // [B, L, D], [B, L], [D, Dh], [Dh, K], [B, Dh] or NULL
    const float *Ain, *dout;               // backward: the kept weights [B, L, K], the arriving gradient [B, K, D]
    float *out, *A;                        // forward outputs
    float *dX, *dc;                        // backward outputs (dc NULL without c)
    float *W1T;    // [Dhp][Dp]: row h holds W1[:, h]
    float *W1P;    // [Dp][Kb]: row d holds W1[d, :]
    float *dPre;   // stacked rows [B L][Dhs]
    float *slab;   // [grid][Dh K]
    int64_t B, nwg;
    int L, D, Dh, K, act, norm, Dp, ld, Dhp, Dhs, Kb, TS, Mv, Mp, nrt;
};

__global__ __launch_bounds__(256) void ap_pack_kernel(ApArgs a, int backward) {
    const int gstride = gridDim.x * 256, g0 = blockIdx.x * 256 + threadIdx.x;
    for (int idx = g0; idx < a.Dhp * a.Dp; idx += gstride) {
        const int d = idx % a.Dp, h = idx / a.Dp;
        a.W1T[idx] = (h < a.Dh && d < a.D) ? a.W1[(int64_t)d * a.Dh + h] : 0.f;
    }
    if (!backward) return;
    for (int idx = g0; idx < a.Dp * a.Kb; idx += gstride) {
        const int h = idx % a.Kb, d = idx / a.Kb;
        a.W1P[idx] = (h < a.Dh && d < a.D) ? a.W1[(int64_t)d * a.Dh + h] : 0.f;
    }
}

// the X tile (zero rows behind the workgroup's samples, zero columns [D, Dp)) and the rows' valid flags
__device__ __forceinline__ void ap_load(const ApArgs &a, int64_t b0, float *XB, float *val) {
    for (int idx = threadIdx.x; idx < a.Mp * a.Dp; idx += blockDim.x) {
        const int m = idx / a.Dp, d = idx % a.Dp;
        const int64_t b = b0 + m / a.L;
        XB[m * a.ld + d] = (m < a.Mv && b < a.B && d < a.D) ? a.X[(b * a.L + m % a.L) * a.D + d] : 0.f;
    }
    for (int m = threadIdx.x; m < a.Mp; m += blockDim.x) {
        const int64_t b = b0 + m / a.L;
        val[m] = (m < a.Mv && b < a.B) ? a.valid[b * a.L + m % a.L] : 0.f;
    }
}

// the hidden values of chunk ch for the wave's 32 rows: hid[q] = act(X W1 + c) at (row rp_mfma32_row(q, h), column ch 32 + i),
// zero in the pad columns
__device__ __forceinline__ void ap_hidden(const ApArgs &a, int64_t b0, const float *XB, int rt, int ch, int i, int h, float (&hid)[16]) {
    const int col = ch * 32 + i;
    f32x16 acc = {0};
    acc = rp_mma_f32_rows(acc, XB + (rt * 32 + i) * a.ld, a.Dp, a.Dp, a.W1T + (int64_t)col * a.Dp, h);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int m = rt * 32 + rp_mfma32_row(q, h);
        const int64_t b = b0 + m / a.L;
        float pre = acc[q];
        if (a.c != nullptr && col < a.Dh && m < a.Mv && b < a.B) pre += a.c[b * a.Dh + col];
        hid[q] = col < a.Dh ? rp_act_apply(a.act, pre) : 0.f;
    }
}

// dynamic LDS: XB [Mp][ld], Sw [4][32][8], S [Mp][8], val [Mp]
__global__ __launch_bounds__(256) void ap_fwd_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ap_lds[];
    float *XB = ap_lds, *Sw = XB + a.Mp * a.ld, *S = Sw + 4 * 32 * 8, *val = S + a.Mp * 8;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int L = a.L, D = a.D, K = a.K;
    const int64_t b0 = (int64_t)blockIdx.x * a.TS;
    ap_load(a, b0, XB, val);
    __syncthreads();
    {
        // the TRANSPOSED product: W1T's rows are the A operand, the X tile's the B operand, so a lane holds ONE row of the
        // tile (m = rt 32 + i) and 16 hidden columns of the chunk: the sum over the chunk's columns is 16 products in the
        // lane and one exchange between the halves of the wave, and the row's scores stay in registers across the chunks
        const int rt = w % a.nrt, nch = a.Dhp / 32, m = rt * 32 + i;
        const int64_t b = b0 + m / L;
        const bool live = m < a.Mv && b < a.B;
        float sacc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sacc[k] = 0.f;
        for (int ch = w / a.nrt; ch < nch; ch += 4 / a.nrt) {
            f32x16 acc = {0};
            acc = rp_mma_f32_rows(acc, a.W1T + (int64_t)(ch * 32 + i) * a.Dp, a.Dp, a.Dp, XB + m * a.ld, h);
            float part[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) part[k] = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int hc = ch * 32 + rp_mfma32_row(q, h);
                if (hc >= a.Dh) continue;
                float pre = acc[q];
                if (a.c != nullptr && live) pre += a.c[b * a.Dh + hc];
                const float hid = rp_act_apply(a.act, pre);
                const float *w2 = a.W2 + hc * K;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < K) part[k] += hid * w2[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sacc[k] += part[k] + __shfl_xor(part[k], 32, 64);  // (the other half's 16 columns)
        }
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) Sw[(w * 32 + i) * 8 + k] = sacc[k];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.Mp * K; idx += blockDim.x) {
        const int m = idx / K, k = idx % K, rt = m / 32;
        float s = 0.f;
        for (int ww = rt; ww < 4; ww += a.nrt) s += Sw[(ww * 32 + m % 32) * 8 + k];
        S[m * 8 + k] = s;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.TS * K; idx += blockDim.x) {
        const int s = idx / K, k = idx % K;
        const int64_t b = b0 + s;
        if (b >= a.B) continue;
        float *sc = S + s * L * 8 + k;
        const float *vl = val + s * L;
        float *Ag = a.A + b * L * K + k;
        if (a.norm == RP_ATTN_POOL_MASK) {
            for (int l = 0; l < L; ++l) {
                const float wgt = sc[l * 8] * vl[l];
                sc[l * 8] = wgt, Ag[l * K] = wgt;
            }
        } else {
            float mx = AP_MASKED, sum = 0.f;
            for (int l = 0; l < L; ++l) {
                const float v = vl[l] != 0.f ? sc[l * 8] : AP_MASKED;
                sc[l * 8] = v, mx = fmaxf(mx, v);
            }
            for (int l = 0; l < L; ++l) {
                const float e = expf(sc[l * 8] - mx);
                sc[l * 8] = e, sum += e;
            }
            const float inv = 1.f / sum;
            for (int l = 0; l < L; ++l) {
                const float wgt = sc[l * 8] * inv;
                sc[l * 8] = wgt, Ag[l * K] = wgt;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.TS * K * D; idx += blockDim.x) {
        const int d = idx % D, k = (idx / D) % K, s = idx / (D * K);
        const int64_t b = b0 + s;
        if (b >= a.B) continue;
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc += S[(s * L + l) * 8 + k] * XB[(s * L + l) * a.ld + d];
        a.out[(b * K + k) * D + d] = acc;
    }
}

// dynamic LDS: XB [Mp][ld], AS [Mp][8], dS [Mp][8], val [Mp], W2s [nrt][Dhp][8]
__global__ __launch_bounds__(256) void ap_bwd_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ap_lds[];
    float *XB = ap_lds, *AS = XB + a.Mp * a.ld, *dS = AS + a.Mp * 8, *val = dS + a.Mp * 8, *W2s = val + a.Mp;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int L = a.L, D = a.D, K = a.K, Dh = a.Dh;
    for (int idx = threadIdx.x; idx < a.nrt * a.Dhp * 8; idx += blockDim.x) W2s[idx] = 0.f;
    for (int64_t grp = blockIdx.x; grp < a.nwg; grp += gridDim.x) {
        const int64_t b0 = grp * a.TS;
        __syncthreads();  // (the tiles of the previous group are free)
        ap_load(a, b0, XB, val);
        for (int idx = threadIdx.x; idx < a.Mp * 8; idx += blockDim.x) {
            const int m = idx / 8, k = idx % 8;
            const int64_t b = b0 + m / L;
            AS[idx] = (m < a.Mv && b < a.B && k < K) ? a.Ain[(b * L + m % L) * K + k] : 0.f;
        }
        __syncthreads();
        // dA[m, k] = dout[b, k, :] . X[m, :]; in mask mode dS = dA valid at once
        for (int idx = threadIdx.x; idx < a.Mp * 8; idx += blockDim.x) {
            const int m = idx / 8, k = idx % 8;
            const int64_t b = b0 + m / L;
            float acc = 0.f;
            if (m < a.Mv && b < a.B && k < K) {
                const float *g = a.dout + (b * K + k) * D, *x = XB + m * a.ld;
                for (int d = 0; d < D; ++d) acc += g[d] * x[d];
                if (a.norm == RP_ATTN_POOL_MASK) acc *= val[m];
            }
            dS[idx] = acc;
        }
        __syncthreads();
        if (a.norm != RP_ATTN_POOL_MASK) {
            for (int idx = threadIdx.x; idx < a.TS * K; idx += blockDim.x) {
                const int s = idx / K, k = idx % K;
                float t = 0.f;
                for (int l = 0; l < L; ++l) t += AS[(s * L + l) * 8 + k] * dS[(s * L + l) * 8 + k];
                for (int l = 0; l < L; ++l) {
                    const int m = s * L + l;
                    dS[m * 8 + k] = val[m] != 0.f ? AS[m * 8 + k] * (dS[m * 8 + k] - t) : 0.f;
                }
            }
            __syncthreads();
        }
        // the chunk walk: dPre to the stacked rows, dW2 to the workgroup's slab
        {
            const int rt = w % a.nrt, nch = a.Dhp / 32;
            float *slab = W2s + rt * a.Dhp * 8;
            for (int ch = w / a.nrt; ch < nch; ch += 4 / a.nrt) {
                float hid[16];
                ap_hidden(a, b0, XB, rt, ch, i, h, hid);
                const int col = ch * 32 + i;
                float w2[8], part[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) w2[k] = (k < K && col < Dh) ? a.W2[col * K + k] : 0.f, part[k] = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int m = rt * 32 + rp_mfma32_row(q, h);
                    const float *ds = dS + m * 8;
                    float dh = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) dh += ds[k] * w2[k], part[k] += hid[q] * ds[k];
                    const int64_t b = b0 + m / L;
                    if (m < a.Mv && b < a.B && col < a.Dhs)
                        a.dPre[(b * L + m % L) * a.Dhs + col] = col < Dh ? rp_act_grad(a.act, dh, hid[q]) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float both = part[k] + __shfl_xor(part[k], 32, 64);  // rows 4 h .. of the two halves of the wave
                    if (h == 0 && k < K) slab[col * 8 + k] += both;
                }
            }
        }
        __syncthreads();  // (the stacked rows of this workgroup are visible to it)
        // dX = A dout + dPre W1^T
        {
            const int nct = a.Dp / 32, ntile = a.nrt * nct;
            for (int tile = w; tile < ntile; tile += 4) {
                const int rt = tile % a.nrt, ct = tile / a.nrt, col = ct * 32 + i;
                f32x16 acc;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int m = rt * 32 + rp_mfma32_row(q, h);
                    const int64_t b = b0 + m / L;
                    float v = 0.f;
                    if (m < a.Mv && b < a.B && col < D)
                        for (int k = 0; k < K; ++k) v += AS[m * 8 + k] * a.dout[(b * K + k) * D + col];
                    acc[q] = v;
                }
                const int mr = rt * 32 + i;
                const int64_t br = b0 + mr / L;
                const float *arow = (mr < a.Mv && br < a.B) ? a.dPre + (br * L + mr % L) * a.Dhs : nullptr;
                acc = rp_mma_f32_rows(acc, arow, a.Kb, a.Dhs, a.W1P + (int64_t)col * a.Kb, h);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int m = rt * 32 + rp_mfma32_row(q, h);
                    const int64_t b = b0 + m / L;
                    if (m < a.Mv && b < a.B && col < D) a.dX[(b * L + m % L) * D + col] = acc[q];
                }
            }
        }
        if (a.dc != nullptr) {
            for (int idx = threadIdx.x; idx < a.TS * Dh; idx += blockDim.x) {
                const int s = idx / Dh, col = idx % Dh;
                const int64_t b = b0 + s;
                if (b >= a.B) continue;
                float acc = 0.f;
                for (int l = 0; l < L; ++l) acc += a.dPre[(b * L + l) * a.Dhs + col];
                a.dc[b * Dh + col] = acc;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < Dh * K; idx += blockDim.x) {
        const int col = idx / K, k = idx % K;
        float s = W2s[col * 8 + k];
        if (a.nrt == 2) s += W2s[(a.Dhp + col) * 8 + k];
        a.slab[(int64_t)blockIdx.x * Dh * K + idx] = s;
    }
}

// dW2[c] = the slabs' sum: 16 threads per element take every 16th slab in order, their partial sums are added in order
__global__ __launch_bounds__(256) void ap_dw2_finish_kernel(const float *__restrict__ slab, int nslab, int n, float *__restrict__ dW2) {
    __shared__ float part[16][16];
    const int e = threadIdx.x & 15, g = threadIdx.x >> 4, c = blockIdx.x * 16 + e;
    float s = 0.f;
    if (c < n)
        for (int q = g; q < nslab; q += 16) s += slab[(int64_t)q * n + c];
    part[g][e] = s;
    __syncthreads();
    if (g != 0 || c >= n) return;
    float t = 0.f;
    for (int j = 0; j < 16; ++j) t += part[j][e];
    dW2[c] = t;
}

bool ap_dims_ok(int L, int D, int Dh, int K) {
    return L >= 1 && L <= AP_MAX_L && D >= 1 && D <= AP_MAX_D && Dh >= 1 && Dh <= AP_MAX_DH && K >= 1 && K <= AP_MAX_K;
}

void ap_shape(int64_t B, int L, int D, int Dh, int K, ApArgs *a) {
    memset(a, 0, sizeof(*a));
    a->B = B, a->L = L, a->D = D, a->Dh = Dh, a->K = K;
    a->Dp = (int)rp_round_up(D, 32), a->ld = a->Dp + 4;
    a->Dhp = (int)rp_round_up(Dh, 32), a->Dhs = (int)rp_round_up(Dh, 4), a->Kb = (int)rp_round_up(a->Dhs, 8);
    a->TS = 64 / L, a->Mv = a->TS * L, a->Mp = (int)rp_round_up(a->Mv, 32), a->nrt = a->Mp / 32;
    a->nwg = rp_cdiv(B, a->TS);
}

size_t ap_lds_fwd(const ApArgs &a) { return 4 * ((size_t)a.Mp * a.ld + 4 * 32 * 8 + (size_t)a.Mp * 9); }
size_t ap_lds_bwd(const ApArgs &a) { return 4 * ((size_t)a.Mp * a.ld + (size_t)a.Mp * 17 + (size_t)a.nrt * a.Dhp * 8); }
// the workgroups of the backward walk ceil(nwg / grid) groups of samples each, all of them about as many
int ap_grid_bwd(const ApArgs &a) { return (int)rp_cdiv(a.nwg, rp_cdiv(a.nwg, AP_SLABS)); }

struct ApWs {
    size_t W1T, W1P, dPre, slab, wgrad, wgrad_bytes, total;
};

int ap_ws(const ApArgs &a, bool bwd, ApWs *o) {
    memset(o, 0, sizeof(*o));
    size_t off = 0;
    o->W1T = off, off += rp_round_up(4 * (size_t)a.Dhp * a.Dp, 256);
    if (bwd) {
        const size_t rows = (size_t)a.B * a.L;
        o->W1P = off, off += rp_round_up(4 * (size_t)a.Dp * a.Kb, 256);
        o->dPre = off, off += rp_round_up(4 * rows * a.Dhs, 256);
        o->slab = off, off += rp_round_up(4 * (size_t)(a.B > 0 ? ap_grid_bwd(a) : 1) * a.Dh * a.K, 256);
        if (rows > 0) {
            const int rc = rp_linear_wgrad_workspace_bytes((int64_t)rows, a.D, a.Dh, &o->wgrad_bytes);
            if (rc != RP_OK) return rc;
        }
        o->wgrad = off, off += rp_round_up(o->wgrad_bytes, 256);
    }
    o->total = off;
    return RP_OK;
}

#define AP_CHECK_DIMS(what)                                                                                                   \
    RP_REQUIRE(B >= 0 && ap_dims_ok(L, D, Dh, K),                                                                             \
               what ": need B >= 0, 1 <= L <= %d, 1 <= D <= %d, 1 <= Dh <= %d, 1 <= K <= %d (got B=%lld L=%d D=%d Dh=%d K=%d)", \
               AP_MAX_L, AP_MAX_D, AP_MAX_DH, AP_MAX_K, (long long)B, L, D, Dh, K);                                           \
    RP_REQUIRE(B * (int64_t)L < ((int64_t)1 << 31) / 4, what ": B L must stay below 2^29")

#define AP_CHECK_MODES(what)                                                                                                \
    RP_REQUIRE(act == RP_ACT_SIGMOID || act == RP_ACT_TANH, what ": act must be RP_ACT_SIGMOID or RP_ACT_TANH (got %d)", act); \
    RP_REQUIRE(norm == RP_ATTN_POOL_MASK || norm == RP_ATTN_POOL_SOFTMAX, what ": norm must be RP_ATTN_POOL_MASK or _SOFTMAX (got %d)", norm)

}  // namespace

extern "C" int rp_attn_pool_geometry(int *max_d, int *max_dh, int *max_k, int *max_l, int *rows_per_workgroup, int *lds_bytes) {
    RP_REQUIRE(max_d && max_dh && max_k && max_l && rows_per_workgroup && lds_bytes, "attn_pool_geometry: null pointer");
    *max_d = AP_MAX_D, *max_dh = AP_MAX_DH, *max_k = AP_MAX_K, *max_l = AP_MAX_L, *rows_per_workgroup = 64;
    *lds_bytes = (int)AP_LDS_MAX;
    return RP_OK;
}

extern "C" int rp_attn_pool_fits(int L, int D, int Dh, int K) {
    if (!ap_dims_ok(L, D, Dh, K)) return 0;
    ApArgs a;
    ap_shape(1, L, D, Dh, K, &a);
    return (ap_lds_fwd(a) <= AP_LDS_MAX && ap_lds_bwd(a) <= AP_LDS_MAX) ? 1 : 0;
}

extern "C" int rp_attn_pool_workspace_bytes(int64_t B, int L, int D, int Dh, int K, int backward, size_t *bytes) {
    RP_REQUIRE(bytes, "attn_pool_workspace_bytes: null pointer");
    AP_CHECK_DIMS("attn_pool_workspace_bytes");
    ApArgs a;
    ap_shape(B, L, D, Dh, K, &a);
    ApWs ws;
    const int rc = ap_ws(a, backward != 0, &ws);
    if (rc != RP_OK) return rc;
    *bytes = ws.total;
    return RP_OK;
}

extern "C" int rp_attn_pool_fwd(const float *X, const float *valid, const float *W1, const float *W2, const float *c, int64_t B,
                                int L, int D, int Dh, int K, int act, int norm, float *out, float *A, void *workspace,
                                size_t workspace_bytes, rp_stream_t stream) {
    AP_CHECK_DIMS("attn_pool_fwd");
    AP_CHECK_MODES("attn_pool_fwd");
    RP_REQUIRE(X && valid && W1 && W2 && out && A && workspace, "attn_pool_fwd: null pointer");
    ApArgs a;
    ap_shape(B, L, D, Dh, K, &a);
    const size_t lds = ap_lds_fwd(a);
    RP_REQUIRE(lds <= AP_LDS_MAX, "attn_pool_fwd: the tile needs %zu bytes of LDS, over %zu", lds, AP_LDS_MAX);
    ApWs ws;
    const int rc = ap_ws(a, false, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "attn_pool_fwd: workspace too small or misaligned");
    if (B == 0) return RP_OK;
    a.X = X, a.valid = valid, a.W1 = W1, a.W2 = W2, a.c = c, a.act = act, a.norm = norm, a.out = out, a.A = A;
    a.W1T = reinterpret_cast<float *>(static_cast<char *>(workspace) + ws.W1T);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_pack_kernel, dim3(32), dim3(256), 0, s, a, 0);
    RP_LAUNCH_CHECK("attn_pool_fwd (weights)");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ap_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ap_fwd_kernel, dim3((unsigned)a.nwg), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("attn_pool_fwd");
    return RP_OK;
}

extern "C" int rp_attn_pool_bwd(const float *X, const float *valid, const float *W1, const float *W2, const float *c,
                                const float *A, const float *dout, int64_t B, int L, int D, int Dh, int K, int act, int norm,
                                float *dX, float *dW1, float *dW2, float *dc, void *workspace, size_t workspace_bytes,
                                rp_stream_t stream) {
    AP_CHECK_DIMS("attn_pool_bwd");
    AP_CHECK_MODES("attn_pool_bwd");
    RP_REQUIRE(X && valid && W1 && W2 && A && dout && dX && dW1 && dW2 && workspace, "attn_pool_bwd: null pointer");
    RP_REQUIRE((c != nullptr) == (dc != nullptr), "attn_pool_bwd: dc goes with c (both or neither)");
    ApArgs a;
    ap_shape(B, L, D, Dh, K, &a);
    const size_t lds = ap_lds_bwd(a);
    RP_REQUIRE(lds <= AP_LDS_MAX, "attn_pool_bwd: the tiles need %zu bytes of LDS, over %zu", lds, AP_LDS_MAX);
    ApWs ws;
    int rc = ap_ws(a, true, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "attn_pool_bwd: workspace too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        (void)hipMemsetAsync(dW1, 0, 4 * (size_t)D * Dh, s);
        (void)hipMemsetAsync(dW2, 0, 4 * (size_t)Dh * K, s);
        return RP_OK;
    }
    char *base = static_cast<char *>(workspace);
    a.X = X, a.valid = valid, a.W1 = W1, a.W2 = W2, a.c = c, a.act = act, a.norm = norm, a.Ain = A, a.dout = dout;
    a.dX = dX, a.dc = dc;
    a.W1T = reinterpret_cast<float *>(base + ws.W1T), a.W1P = reinterpret_cast<float *>(base + ws.W1P);
    a.dPre = reinterpret_cast<float *>(base + ws.dPre), a.slab = reinterpret_cast<float *>(base + ws.slab);
    hipLaunchKernelGGL(ap_pack_kernel, dim3(32), dim3(256), 0, s, a, 1);
    RP_LAUNCH_CHECK("attn_pool_bwd (weights)");
    const int grid = ap_grid_bwd(a);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ap_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ap_bwd_kernel, dim3((unsigned)grid), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("attn_pool_bwd");
    hipLaunchKernelGGL(ap_dw2_finish_kernel, dim3((unsigned)rp_cdiv(Dh * K, 16)), dim3(256), 0, s, a.slab, grid, Dh * K, dW2);
    RP_LAUNCH_CHECK("attn_pool_bwd (dW2)");
    // dW1 [D, Dh] = X^T dPre over the stacked rows
    return rp_linear_wgrad(X, D, a.dPre, a.Dhs, dW1, Dh, nullptr, B * L, D, Dh, 0, base + ws.wgrad, ws.wgrad_bytes, stream);
}
