// Residual blocks of NextItNet, gfx950 — replaces ResBlockTwoMasked / ResBlockOneMasked of rec_pangu/models/layers/conv.py
// (dilated causal nn.Conv1d on a left-padded [B, C, L] tensor, the file's own channel LayerNorm, ReLU, residual) and their
// autograd.  One launch per block and direction runs every stage of the block on an LDS-resident tile.
//
// VIRTUAL SEQUENCE.  A launch works on R rows per sample; row r stands for source position
//     pos(r) = anchor_b - (R - 1 - r) stride.
//   pos(r) < 0      causal padding: the row is zero at the input of EVERY conv of the block (a LayerNorm stage writes zeros
//                   there), as the reference pads each conv's own input;
//   pos(r) >= len_b the row is LOADED as zero (the reference's masked_fill) and is an ordinary row from then on;
//   the residual adds the loaded row.
//   full mode: stride 1, R = L, anchor L - 1, internal dilations the block's own, all [B, L, C] rows are written;
//   last mode: stride = the block's dilation d, anchor len_b - 1 (L - 1 for an empty row), internal dilations (1, 2) over
//              R = 3 (k - 1) + 1 rows (two-masked) or 1 over R = k rows (one-masked): the rows the read position depends on,
//              gathered; [B, C] is written, the last virtual row.
//
// STAGES.  Two device functions each way, composed per block type:
//   cc_conv    Cin -> Cout, k taps at dilation delta over the tile: a matrix product with K = k Cin whose A operand for tap j is
//              the same LDS tile read (k - 1 - j) delta rows earlier (zero in front of the sample's first row), on the exact-fp32
//              matrix core (v_mfma_f32_32x32x2_f32); weights from zero-padded copies [k][Cout_p][Cin_p] (one small launch per
//              call), read through L2.  With dir = -1 and the transposed copies it is the conv's input gradient.
//   cc_ln      channel LayerNorm (biased variance, eps 1e-5) + ReLU per row, one wave per row, lane sums from device.h.
//   two-masked: conv0 LN0 conv1 LN1 (+ x);   one-masked: LN0 conv0(1x1) LN1 conv1 LN2 conv2(1x1) (+ x).
// A workgroup of 256 threads owns TS samples (TS R <= 64 rows, or one sample), rows padded to a multiple of 32; two tile
// buffers [Mp][Cp + 4] ping-pong (the + 4 keeps the 32 rows of an A read on distinct bank groups; a tap's shift moves all
// lanes alike, so a dilation equal to the bank period costs nothing).
//
// BACKWARD.  One launch recomputes the stages from the block's input, leaving in the workspace each LayerNorm's input
// [B R, Cout] and each conv's input as tap-stacked rows [B R, Cin k] (column ci k + j, zero where a tap reads padding),
// then walks the stages in reverse with the gradient in LDS; each LayerNorm's input is overwritten by the conv's
// pre-activation gradient.  dW [Cout, Cin, k] is then ONE rp_linear_wgrad per conv (the stacking order is the weight's own
// layout), the conv bias its column sums; gamma / beta gradients are summed per workgroup in row order into slabs and added
// in workgroup order by a second launch.  dX: every position of the sample is written by the workgroup that owns it (zero
// where no virtual row stands, and at positions >= len_b).  No floating-point atomics: two runs give the same bits.
// Launches: forward 2 (repack + block); backward 3 + 2 convs = 7 (two-masked) or 9 (one-masked), whatever B is.
#include "common.h"

namespace {

constexpr int CC_MAX_C = 128, CC_MAX_K = 5, CC_MAX_L = 128, CC_MAX_LC = 8192;
constexpr size_t CC_LDS_MAX = 160 * 1024 - 512;
constexpr float CC_EPS = 1e-5f;

struct CcArgs {
    const float *X;       // [B, L, C]
    const int64_t *lens;  // [B]
    const float *dout;    // full: [B, L, C]; last: [B, C]
    float *out;           // full: [B, L, C]; last: [B, C]
    float *dX;            // [B, L, C]
    int64_t B;
    int L, C, R, last, one, nconv, TS, Mv, Mp, ld, Wp;
    int64_t stride;
    int cin[3], cout[3], cinp[3], coutp[3], taps[3], dil[3];
    const float *w[3];    // the parameters themselves (repack only)
    float *wp[3];         // [taps][coutp][cinp]
    float *wt[3];         // [taps][cinp][coutp]
    const float *cb[3], *lg[3], *lb[3];
    float *A[3];          // conv c's output (a LayerNorm's input), then the conv's pre-activation gradient: [B R, cout]
    float *S[3];          // conv c's input, tap-stacked: [B R, cin taps] (one-masked conv2 in last mode: [B, cin])
    float *slab;          // [workgroups][slabw]
    int slabw, lnw[3], lnoff[3];
    float *dlg[3], *dlb[3];
    int64_t nslab;
};

__global__ __launch_bounds__(256) void cc_pack_kernel(CcArgs a) {
    for (int c = 0; c < a.nconv; ++c) {
        const int n = a.taps[c] * a.coutp[c] * a.cinp[c];
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
            const int ci = idx % a.cinp[c], co = (idx / a.cinp[c]) % a.coutp[c], j = idx / (a.cinp[c] * a.coutp[c]);
            const float v = (ci < a.cin[c] && co < a.cout[c]) ? a.w[c][((int64_t)co * a.cin[c] + ci) * a.taps[c] + j] : 0.f;
            a.wp[c][idx] = v;
            a.wt[c][((int64_t)j * a.cinp[c] + ci) * a.coutp[c] + co] = v;
        }
    }
}

// per tile row m = s R + r: live (a row of the virtual sequence at pos >= 0), grow = b R + r (-1: no such sample), gsrc = the
// source row b L + pos of X (-1: loaded as zero)
__device__ __forceinline__ void cc_rows(const CcArgs &a, int64_t b0, int *live, int *grow, int *gsrc) {
    for (int m = threadIdx.x; m < a.Mp; m += blockDim.x) {
        const int s = m / a.R, r = m % a.R;
        const int64_t b = b0 + s;
        int lv = 0, gr = -1, gs = -1;
        if (s < a.TS && b < a.B) {
            int64_t len = a.lens[b];
            len = len < 0 ? 0 : (len > a.L ? a.L : len);
            const int64_t anchor = (a.last && len > 0) ? len - 1 : a.L - 1;
            const int64_t pos = anchor - (int64_t)(a.R - 1 - r) * a.stride;
            gr = (int)(b * a.R + r);
            lv = pos >= 0;
            if (pos >= 0 && pos < len) gs = (int)(b * a.L + pos);
        }
        live[m] = lv, grow[m] = gr, gsrc[m] = gs;
    }
}

// the loaded rows -> buf [Mp][ld], zero-padded to Wp columns
__device__ __forceinline__ void cc_load_x(const CcArgs &a, float *buf, const int *gsrc) {
    for (int idx = threadIdx.x; idx < a.Mp * a.Wp; idx += blockDim.x) {
        const int m = idx / a.Wp, c = idx % a.Wp;
        const int gs = gsrc[m];
        buf[m * a.ld + c] = (gs >= 0 && c < a.C) ? a.X[(int64_t)gs * a.C + c] : 0.f;
    }
}

// dst [Mp][nout_p] = sum over taps of src shifted by dir (taps - 1 - j) dil rows inside its sample, times W [taps][nout_p][nin_p]
__device__ __forceinline__ void cc_conv(const float *src, float *dst, int ld, int Mv, int Mp, int R, int nin_p, int nout_p,
                                        int nout, int taps, int dil, int dir, const float *__restrict__ W,
                                        const float *__restrict__ bias) {
    const int tid = threadIdx.x, w = tid >> 6, nw = blockDim.x >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int nrt = Mp / 32, ntile = nrt * (nout_p / 32);
    for (int t = w; t < ntile; t += nw) {
        const int rt = t % nrt, ct = t / nrt;
        const int m = rt * 32 + i, r = m % R, col = ct * 32 + i;
        f32x16 acc = {0};
        for (int j = 0; j < taps; ++j) {
            const int shift = dir * (taps - 1 - j) * dil;
            const int rs = r - shift;
            const bool ok = m < Mv && rs >= 0 && rs < R;
            if (!__any(ok)) continue;  // (uniform over the wave)
            const float *arow = src + (ok ? m - shift : m) * ld;
            const float *wrow = W + (int64_t)(j * nout_p + col) * nin_p;
            for (int kq = 0; kq < nin_p / 8; ++kq) {
                const int k = kq * 8 + 4 * h;
                f32x4 a4 = *reinterpret_cast<const f32x4 *>(arow + k);
                if (!ok) a4 = f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 b4 = *reinterpret_cast<const f32x4 *>(wrow + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc, 0, 0, 0);
            }
        }
        const float bv = (bias != nullptr && col < nout) ? bias[col] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) dst[(rt * 32 + rp_mfma32_row(q, h)) * ld + col] = acc[q] + bv;
    }
}

// in place: relu(gamma (x - mean) / sqrt(var + eps) + beta) over the n channels of each row, zeros on rows that are not live
// and in columns [n, Wp); spill != NULL keeps the stage's input [grow, n]
__device__ __forceinline__ void cc_ln(float *buf, int ld, int Mp, int Wp, int n, const float *__restrict__ g,
                                      const float *__restrict__ be, const int *live, const int *grow, float *__restrict__ spill) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int c0 = lane, c1 = lane + 64;
    const float g0 = c0 < n ? g[c0] : 0.f, g1 = c1 < n ? g[c1] : 0.f, e0 = c0 < n ? be[c0] : 0.f, e1 = c1 < n ? be[c1] : 0.f;
    for (int m = w; m < Mp; m += nw) {
        float *row = buf + m * ld;
        float y0 = 0.f, y1 = 0.f;
        if (live[m]) {
            const float v0 = c0 < n ? row[c0] : 0.f, v1 = c1 < n ? row[c1] : 0.f;
            if (spill != nullptr && grow[m] >= 0) {
                if (c0 < n) spill[(int64_t)grow[m] * n + c0] = v0;
                if (c1 < n) spill[(int64_t)grow[m] * n + c1] = v1;
            }
            const float mean = rp_lane_sum(v0 + v1) / (float)n;
            const float d0 = c0 < n ? v0 - mean : 0.f, d1 = c1 < n ? v1 - mean : 0.f;
            const float den = sqrtf(rp_lane_sum(d0 * d0 + d1 * d1) / (float)n + CC_EPS);
            y0 = fmaxf(d0 / den * g0 + e0, 0.f), y1 = fmaxf(d1 / den * g1 + e1, 0.f);
        }
        if (c0 < Wp) row[c0] = c0 < n ? y0 : 0.f;
        if (c1 < Wp) row[c1] = c1 < n ? y1 : 0.f;
    }
}

// in place: the gradient of cc_ln's input from the gradient of its output (gbuf) and its input (rows of asrc: [grow, n], or X's
// rows through gsrc when from_x); zeros on rows that are not live.  G != NULL also keeps the result [grow, n].  gamma / beta
// gradients: per lane in row order, the waves added in wave order through red [nw][2][128], into this workgroup's slab.
__device__ __forceinline__ void cc_ln_bwd(float *gbuf, int ld, int Mp, int Wp, int n, const float *__restrict__ g,
                                          const float *__restrict__ be, const int *live, const int *grow, const int *gsrc,
                                          const float *asrc, bool from_x, float *G, float *red, float *__restrict__ slab) {
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int c0 = lane, c1 = lane + 64;
    const float g0 = c0 < n ? g[c0] : 0.f, g1 = c1 < n ? g[c1] : 0.f, e0 = c0 < n ? be[c0] : 0.f, e1 = c1 < n ? be[c1] : 0.f;
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    for (int m = w; m < Mp; m += nw) {
        float *row = gbuf + m * ld;
        float r0 = 0.f, r1 = 0.f;
        if (live[m]) {
            float v0 = 0.f, v1 = 0.f;
            const int64_t at = from_x ? gsrc[m] : grow[m];
            if (at >= 0) {
                if (c0 < n) v0 = asrc[at * n + c0];
                if (c1 < n) v1 = asrc[at * n + c1];
            }
            const float mean = rp_lane_sum(v0 + v1) / (float)n;
            const float d0 = c0 < n ? v0 - mean : 0.f, d1 = c1 < n ? v1 - mean : 0.f;
            const float den = sqrtf(rp_lane_sum(d0 * d0 + d1 * d1) / (float)n + CC_EPS);
            const float x0 = d0 / den, x1 = d1 / den;
            const float dy0 = (c0 < n && x0 * g0 + e0 > 0.f) ? row[c0] : 0.f, dy1 = (c1 < n && x1 * g1 + e1 > 0.f) ? row[c1] : 0.f;
            db0 += dy0, db1 += dy1, dg0 += dy0 * x0, dg1 += dy1 * x1;
            const float h0 = dy0 * g0, h1 = dy1 * g1;
            const float s1 = rp_lane_sum(h0 + h1) / (float)n, s2 = rp_lane_sum(h0 * x0 + h1 * x1) / (float)n;
            r0 = c0 < n ? (h0 - s1 - x0 * s2) / den : 0.f, r1 = c1 < n ? (h1 - s1 - x1 * s2) / den : 0.f;
        }
        if (c0 < Wp) row[c0] = r0;
        if (c1 < Wp) row[c1] = r1;
        if (G != nullptr && grow[m] >= 0) {
            if (c0 < n) G[(int64_t)grow[m] * n + c0] = r0;
            if (c1 < n) G[(int64_t)grow[m] * n + c1] = r1;
        }
    }
    red[(w * 2 + 0) * 128 + c0] = dg0, red[(w * 2 + 0) * 128 + c1] = dg1;
    red[(w * 2 + 1) * 128 + c0] = db0, red[(w * 2 + 1) * 128 + c1] = db1;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * n; idx += blockDim.x) {
        const int which = idx / n, c = idx % n;
        float s = 0.f;
        for (int q = 0; q < nw; ++q) s += red[(q * 2 + which) * 128 + c];
        slab[idx] = s;
    }
    __syncthreads();
}

// conv c's input as tap-stacked rows: S[grow, ci taps + j] = src[row - (taps - 1 - j) dil, ci], zero in front of the sample
__device__ __forceinline__ void cc_stack(const CcArgs &a, int c, const float *src, const int *grow) {
    const int taps = a.taps[c], K = a.cin[c] * taps;
    const bool last_only = a.last && a.one && c == 2;
    float *S = a.S[c];
    for (int idx = threadIdx.x; idx < a.Mv * K; idx += blockDim.x) {
        const int m = idx / K, q = idx % K, ci = q / taps, j = q % taps, r = m % a.R;
        const int gr = grow[m];
        if (gr < 0 || (last_only && r != a.R - 1)) continue;
        const int shift = (taps - 1 - j) * a.dil[c];
        const float v = r - shift >= 0 ? src[(m - shift) * a.ld + ci] : 0.f;
        S[(int64_t)(last_only ? gr / a.R : gr) * K + q] = v;
    }
}

// every stage of the block over the workgroup's tile -> the buffer that holds the result in front of the residual
template <bool KEEP>
__device__ __forceinline__ float *cc_forward(const CcArgs &a, float *P0, float *P1, const int *live, const int *grow,
                                             const int *gsrc) {
    cc_load_x(a, P0, gsrc);
    __syncthreads();
    float *cur = P0, *oth = P1;
    if (a.one) {
        cc_ln(cur, a.ld, a.Mp, a.Wp, a.C, a.lg[0], a.lb[0], live, grow, nullptr);
        __syncthreads();
    }
    for (int c = 0; c < a.nconv; ++c) {
        if (KEEP) cc_stack(a, c, cur, grow);
        cc_conv(cur, oth, a.ld, a.Mv, a.Mp, a.R, a.cinp[c], a.coutp[c], a.cout[c], a.taps[c], a.dil[c], 1, a.wp[c], a.cb[c]);
        __syncthreads();
        float *t = cur;
        cur = oth, oth = t;
        const int ln = c + a.one;
        if (!a.one || c < 2) {
            cc_ln(cur, a.ld, a.Mp, a.Wp, a.cout[c], a.lg[ln], a.lb[ln], live, grow, KEEP ? a.A[c] : nullptr);
            __syncthreads();
        }
    }
    return cur;
}

// dynamic LDS: P0, P1 [Mp][ld] floats, live / grow / gsrc [Mp] ints (+ red [4][2][128] floats in the backward)
__global__ __launch_bounds__(256) void cc_fwd_kernel(CcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];
    float *P0 = cc_lds, *P1 = P0 + a.Mp * a.ld;
    int *live = reinterpret_cast<int *>(P1 + a.Mp * a.ld), *grow = live + a.Mp, *gsrc = grow + a.Mp;
    const int64_t b0 = (int64_t)blockIdx.x * a.TS;
    cc_rows(a, b0, live, grow, gsrc);
    __syncthreads();
    const float *res = cc_forward<false>(a, P0, P1, live, grow, gsrc);
    for (int idx = threadIdx.x; idx < a.Mv * a.C; idx += blockDim.x) {
        const int m = idx / a.C, c = idx % a.C;
        const int gr = grow[m], gs = gsrc[m];
        if (gr < 0 || (a.last && m % a.R != a.R - 1)) continue;
        const float v = res[m * a.ld + c] + (gs >= 0 ? a.X[(int64_t)gs * a.C + c] : 0.f);
        a.out[(int64_t)(a.last ? gr / a.R : gr) * a.C + c] = v;
    }
}

__global__ __launch_bounds__(256) void cc_bwd_kernel(CcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];
    float *P0 = cc_lds, *P1 = P0 + a.Mp * a.ld;
    int *live = reinterpret_cast<int *>(P1 + a.Mp * a.ld), *grow = live + a.Mp, *gsrc = grow + a.Mp;
    float *red = reinterpret_cast<float *>(gsrc + a.Mp);
    const int64_t b0 = (int64_t)blockIdx.x * a.TS;
    float *slab = a.slab + (int64_t)blockIdx.x * a.slabw;
    cc_rows(a, b0, live, grow, gsrc);
    __syncthreads();
    float *oth = cc_forward<true>(a, P0, P1, live, grow, gsrc);
    float *cur = oth == P0 ? P1 : P0;
    // the arriving gradient as a tile: every row in full mode, the last virtual row alone in last mode
    for (int idx = threadIdx.x; idx < a.Mp * a.Wp; idx += blockDim.x) {
        const int m = idx / a.Wp, c = idx % a.Wp;
        const int gr = grow[m];
        float v = 0.f;
        if (gr >= 0 && c < a.C && live[m]) {
            if (!a.last) v = a.dout[(int64_t)gr * a.C + c];
            else if (m % a.R == a.R - 1) v = a.dout[(int64_t)(gr / a.R) * a.C + c];
        }
        cur[m * a.ld + c] = v;
    }
    __syncthreads();
    for (int c = a.nconv - 1; c >= 0; --c) {
        const int ln = c + a.one;
        if (!a.one || c < 2) {
            cc_ln_bwd(cur, a.ld, a.Mp, a.Wp, a.cout[c], a.lg[ln], a.lb[ln], live, grow, gsrc, a.A[c], false, a.A[c], red,
                      slab + a.lnoff[ln]);
        }
        cc_conv(cur, oth, a.ld, a.Mv, a.Mp, a.R, a.coutp[c], a.cinp[c], a.cin[c], a.taps[c], a.dil[c], -1, a.wt[c], nullptr);
        __syncthreads();
        float *t = cur;
        cur = oth, oth = t;
    }
    if (a.one) cc_ln_bwd(cur, a.ld, a.Mp, a.Wp, a.C, a.lg[0], a.lb[0], live, grow, gsrc, a.X, true, nullptr, red, slab + a.lnoff[0]);
    // dX: every position of the workgroup's samples, one writer each
    for (int idx = threadIdx.x; idx < a.TS * a.L * a.C; idx += blockDim.x) {
        const int c = idx % a.C, p = (idx / a.C) % a.L, s = idx / (a.C * a.L);
        const int64_t b = b0 + s;
        if (b >= a.B) continue;
        int64_t len = a.lens[b];
        len = len < 0 ? 0 : (len > a.L ? a.L : len);
        const int64_t anchor = (a.last && len > 0) ? len - 1 : a.L - 1, q = anchor - p;
        float v = 0.f;
        if (p < len && q >= 0 && q % a.stride == 0 && q / a.stride < a.R) {
            const int r = a.R - 1 - (int)(q / a.stride);
            v = cur[(s * a.R + r) * a.ld + c];
            if (!a.last) v += a.dout[((int64_t)b * a.L + p) * a.C + c];
            else if (r == a.R - 1) v += a.dout[(int64_t)b * a.C + c];
        }
        a.dX[((int64_t)b * a.L + p) * a.C + c] = v;
    }
}

// gamma / beta gradients: the workgroups' slabs added in workgroup order (16 waves take 16 consecutive runs of slabs, the
// runs are then added in run order); one workgroup per 64 slab columns
__global__ __launch_bounds__(1024) void cc_finish_kernel(CcArgs a) {
    __shared__ float part[16][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, e = blockIdx.x * 64 + lane;
    const int64_t run = (a.nslab + 15) / 16, q0 = w * run, q1 = q0 + run < a.nslab ? q0 + run : a.nslab;
    float s = 0.f;
    if (e < a.slabw)
        for (int64_t q = q0; q < q1; ++q) s += a.slab[q * a.slabw + e];
    part[w][lane] = s;
    __syncthreads();
    if (w != 0 || e >= a.slabw) return;
    float t = 0.f;
    for (int q = 0; q < 16; ++q) t += part[q][lane];
    for (int ln = 0; ln < 3; ++ln) {
        if (a.lnw[ln] == 0) continue;
        const int off = e - a.lnoff[ln];
        if (off >= 0 && off < a.lnw[ln]) a.dlg[ln][off] = t;
        else if (off >= a.lnw[ln] && off < 2 * a.lnw[ln]) a.dlb[ln][off - a.lnw[ln]] = t;
    }
}

struct CcWs {
    size_t wp[3], wt[3], A[3], S[3], slab, wgrad, wgrad_bytes, total;
};

bool cc_dims_ok(int L, int C, int k, int one) {
    return C >= 2 && C <= CC_MAX_C && k >= 1 && k <= CC_MAX_K && L >= 1 && L <= CC_MAX_L && (int64_t)L * C <= CC_MAX_LC &&
           (!one || C / 2 >= 1);
}

// the launch's shape (everything but pointers); dilation >= 1
void cc_shape(int64_t B, int L, int C, int k, int64_t dilation, int one, int last, CcArgs *a) {
    memset(a, 0, sizeof(*a));
    a->B = B, a->L = L, a->C = C, a->last = last, a->one = one;
    const int d = (int)(dilation > L ? L : dilation);  // (a shift of L rows or more reads padding whatever it is)
    if (one) {
        const int mid = C / 2;
        a->nconv = 3;
        const int cin[3] = {C, mid, mid}, cout[3] = {mid, mid, C}, taps[3] = {1, k, 1}, dil[3] = {1, last ? 1 : d, 1};
        for (int c = 0; c < 3; ++c) a->cin[c] = cin[c], a->cout[c] = cout[c], a->taps[c] = taps[c], a->dil[c] = dil[c];
        a->R = last ? k : L;
        a->lnw[0] = C, a->lnw[1] = mid, a->lnw[2] = mid;
    } else {
        a->nconv = 2;
        for (int c = 0; c < 2; ++c) a->cin[c] = C, a->cout[c] = C, a->taps[c] = k;
        a->dil[0] = last ? 1 : d, a->dil[1] = last ? 2 : 2 * d;
        a->R = last ? 3 * (k - 1) + 1 : L;
        a->lnw[0] = C, a->lnw[1] = C;
    }
    a->stride = last ? dilation : 1;
    for (int c = 0; c < a->nconv; ++c) a->cinp[c] = (int)rp_round_up(a->cin[c], 32), a->coutp[c] = (int)rp_round_up(a->cout[c], 32);
    int off = 0;
    for (int ln = 0; ln < 3; ++ln) a->lnoff[ln] = off, off += 2 * a->lnw[ln];
    a->slabw = off;
    a->TS = a->R >= 64 ? 1 : 64 / a->R;
    a->Mv = a->TS * a->R, a->Mp = (int)rp_round_up(a->Mv, 32);
    a->Wp = (int)rp_round_up(C, 32), a->ld = a->Wp + 4;
    a->nslab = rp_cdiv(B, a->TS);
}

size_t cc_lds_bytes(const CcArgs &a, bool bwd) {
    return sizeof(float) * 2 * (size_t)a.Mp * a.ld + sizeof(int) * 3 * (size_t)a.Mp + (bwd ? sizeof(float) * 4 * 2 * 128 : 0);
}

int cc_ws(const CcArgs &a, bool bwd, CcWs *o) {
    size_t off = 0;
    memset(o, 0, sizeof(*o));
    const size_t rows = (size_t)a.B * a.R;
    for (int c = 0; c < a.nconv; ++c) {
        const size_t n = rp_round_up(sizeof(float) * a.taps[c] * a.coutp[c] * a.cinp[c], 256);
        o->wp[c] = off, off += n;
        o->wt[c] = off, off += n;
    }
    if (bwd) {
        for (int c = 0; c < a.nconv; ++c) {
            const bool last_only = a.last && a.one && c == 2;
            o->A[c] = off, off += (!a.one || c < 2) ? rp_round_up(sizeof(float) * rows * a.cout[c], 256) : 0;
            o->S[c] = off, off += rp_round_up(sizeof(float) * (last_only ? (size_t)a.B : rows) * a.cin[c] * a.taps[c], 256);
            size_t wb = 0;
            const int rc = rp_linear_wgrad_workspace_bytes(last_only ? a.B : (int64_t)rows, a.cout[c], a.cin[c] * a.taps[c], &wb);
            if (rc != RP_OK) return rc;
            o->wgrad_bytes = wb > o->wgrad_bytes ? wb : o->wgrad_bytes;
        }
        o->slab = off, off += rp_round_up(sizeof(float) * (size_t)a.nslab * a.slabw, 256);
        o->wgrad = off, off += rp_round_up(o->wgrad_bytes, 256);
    }
    o->total = off;
    return RP_OK;
}

#define CC_CHECK_DIMS(what)                                                                                                  \
    RP_REQUIRE(B >= 0 && dilation >= 1 && cc_dims_ok(L, C, k, one_masked),                                                   \
               what ": need B >= 0, dilation >= 1, 2 <= C <= %d, 1 <= k <= %d, 1 <= L <= %d and L C <= %d (got B=%lld L=%d " \
                    "C=%d k=%d dilation=%lld)",                                                                             \
               CC_MAX_C, CC_MAX_K, CC_MAX_L, CC_MAX_LC, (long long)B, L, C, k, (long long)dilation);                         \
    RP_REQUIRE(B * (int64_t)(L > 16 ? L : 16) < ((int64_t)1 << 31), what ": B L must stay below 2^31")

// params / grads: 12 pointers, conv weight 0..2, conv bias 0..2, LayerNorm gamma 0..2, beta 0..2 in stage order
int cc_bind(CcArgs *a, const float *const *params, float *const *grads, void *workspace, const CcWs &ws, const char *what) {
    char *base = static_cast<char *>(workspace);
    for (int c = 0; c < a->nconv; ++c) {
        RP_REQUIRE(params[c] && params[3 + c], "%s: null conv parameter", what);
        a->w[c] = params[c], a->cb[c] = params[3 + c];
        a->wp[c] = reinterpret_cast<float *>(base + ws.wp[c]), a->wt[c] = reinterpret_cast<float *>(base + ws.wt[c]);
        a->A[c] = reinterpret_cast<float *>(base + ws.A[c]), a->S[c] = reinterpret_cast<float *>(base + ws.S[c]);
        RP_REQUIRE(grads == nullptr || (grads[c] && grads[3 + c]), "%s: null conv gradient", what);
    }
    for (int ln = 0; ln < 3; ++ln) {
        if (a->lnw[ln] == 0) continue;
        RP_REQUIRE(params[6 + ln] && params[9 + ln], "%s: null LayerNorm parameter", what);
        a->lg[ln] = params[6 + ln], a->lb[ln] = params[9 + ln];
        if (grads != nullptr) {
            RP_REQUIRE(grads[6 + ln] && grads[9 + ln], "%s: null LayerNorm gradient", what);
            a->dlg[ln] = grads[6 + ln], a->dlb[ln] = grads[9 + ln];
        }
    }
    a->slab = reinterpret_cast<float *>(base + ws.slab);
    return RP_OK;
}

}  // namespace

extern "C" int rp_causal_conv_geometry(int *max_c, int *max_k, int *max_l, int *max_lc, int *lds_bytes) {
    RP_REQUIRE(max_c && max_k && max_l && max_lc && lds_bytes, "causal_conv_geometry: null pointer");
    *max_c = CC_MAX_C, *max_k = CC_MAX_K, *max_l = CC_MAX_L, *max_lc = CC_MAX_LC, *lds_bytes = (int)CC_LDS_MAX;
    return RP_OK;
}

extern "C" int rp_causal_conv_fits(int L, int C, int k, int one_masked) {
    if (!cc_dims_ok(L, C, k, one_masked)) return 0;
    CcArgs a;
    for (int last = 0; last < 2; ++last) {
        cc_shape(1, L, C, k, 1, one_masked, last, &a);
        if (cc_lds_bytes(a, true) > CC_LDS_MAX) return 0;
    }
    return 1;
}

extern "C" int rp_causal_conv_workspace_bytes(int64_t B, int L, int C, int k, int one_masked, int last, int backward,
                                              size_t *bytes) {
    RP_REQUIRE(bytes, "causal_conv_workspace_bytes: null pointer");
    const int64_t dilation = 1;
    CC_CHECK_DIMS("causal_conv_workspace_bytes");
    CcArgs a;
    cc_shape(B, L, C, k, 1, one_masked, last, &a);
    CcWs ws;
    const int rc = cc_ws(a, backward != 0, &ws);
    if (rc != RP_OK) return rc;
    *bytes = ws.total;
    return RP_OK;
}

extern "C" int rp_causal_conv_fwd(const float *X, const int64_t *lens, int64_t B, int L, int C, int k, int64_t dilation,
                                  int one_masked, int last, const float *const *params, float *out, void *workspace,
                                  size_t workspace_bytes, rp_stream_t stream) {
    CC_CHECK_DIMS("causal_conv_fwd");
    RP_REQUIRE(X && lens && params && out && workspace, "causal_conv_fwd: null pointer");
    CcArgs a;
    cc_shape(B, L, C, k, dilation, one_masked, last, &a);
    const size_t lds = cc_lds_bytes(a, false);
    RP_REQUIRE(lds <= CC_LDS_MAX, "causal_conv_fwd: the tile needs %zu bytes of LDS, over %zu", lds, CC_LDS_MAX);
    CcWs ws;
    int rc = cc_ws(a, false, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "causal_conv_fwd: workspace too small or misaligned");
    rc = cc_bind(&a, params, nullptr, workspace, ws, "causal_conv_fwd");
    if (rc != RP_OK) return rc;
    if (B == 0) return RP_OK;
    a.X = X, a.lens = lens, a.out = out;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_pack_kernel, dim3(64), dim3(256), 0, s, a);
    RP_LAUNCH_CHECK("causal_conv_fwd (weights)");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cc_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(cc_fwd_kernel, dim3((unsigned)a.nslab), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("causal_conv_fwd");
    return RP_OK;
}

extern "C" int rp_causal_conv_bwd(const float *X, const int64_t *lens, const float *dout, int64_t B, int L, int C, int k,
                                  int64_t dilation, int one_masked, int last, const float *const *params, float *dX,
                                  float *const *grads, void *workspace, size_t workspace_bytes, rp_stream_t stream) {
    CC_CHECK_DIMS("causal_conv_bwd");
    RP_REQUIRE(X && lens && dout && params && dX && grads && workspace, "causal_conv_bwd: null pointer");
    CcArgs a;
    cc_shape(B, L, C, k, dilation, one_masked, last, &a);
    const size_t lds = cc_lds_bytes(a, true);
    RP_REQUIRE(lds <= CC_LDS_MAX, "causal_conv_bwd: the tile needs %zu bytes of LDS, over %zu", lds, CC_LDS_MAX);
    CcWs ws;
    int rc = cc_ws(a, true, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "causal_conv_bwd: workspace too small or misaligned");
    rc = cc_bind(&a, params, grads, workspace, ws, "causal_conv_bwd");
    if (rc != RP_OK) return rc;
    if (B == 0) return RP_OK;
    a.X = X, a.lens = lens, a.dout = dout, a.dX = dX;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_pack_kernel, dim3(64), dim3(256), 0, s, a);
    RP_LAUNCH_CHECK("causal_conv_bwd (weights)");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cc_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(cc_bwd_kernel, dim3((unsigned)a.nslab), dim3(256), (unsigned)lds, s, a);
    RP_LAUNCH_CHECK("causal_conv_bwd");
    char *base = static_cast<char *>(workspace);
    for (int c = 0; c < a.nconv; ++c) {
        const bool last_only = a.last && a.one && c == 2;
        const int K = a.cin[c] * a.taps[c];
        const float *dy = (a.one && c == 2) ? dout : a.A[c];  // (the 1x1 conv in front of the residual: the arriving rows)
        rc = rp_linear_wgrad(dy, a.cout[c], a.S[c], K, grads[c], K, grads[3 + c], last_only ? B : B * a.R, a.cout[c], K, 0,
                             base + ws.wgrad, ws.wgrad_bytes, stream);
        if (rc != RP_OK) return rc;
    }
    hipLaunchKernelGGL(cc_finish_kernel, dim3((unsigned)rp_cdiv(a.slabw, 64)), dim3(1024), 0, s, a);
    RP_LAUNCH_CHECK("causal_conv_bwd (gamma, beta)");
    return RP_OK;
}
