// CCPM's conv + k-max-pooling + tanh stack (ranking/ccpm.py:77-107) as one launch each way, fp32, gfx950.
//
// rp_ccpm_*  reference, per layer: ZeroPad2d((0, 0, kh - 1, kh - 1)) -> Conv2d(C_in, C_out, (kh, 1)) -> KMaxPooling(k, dim=2)
//            (topk -> sort the indices -> gather) -> Tanh, over [B, C, L, D].  Every conv kernel is (kh, 1) and the pooling
//            runs along L, so no step mixes two embedding columns: for a fixed (sample b, column d) the whole stack is a small
//            function of the F floats x[b, :, d].  One THREAD owns one column: it holds the column's activations in LDS and
//            walks the layers; nothing of size B C L D reaches global memory, forward or backward.
//
// Mapping.  Columns are numbered c = b D + d; a workgroup is ONE wave of 64 consecutive columns (a field's D floats of a row
// are contiguous, so the 64 loads of a field coalesce) and walks the 64-column tiles with the stride of its grid.  Every
// per-thread array lives in LDS as [slot][thread] (slot stride 64 floats: consecutive lanes on consecutive banks, no
// conflict, and no run-time-indexed private array, hence no scratch).  A thread only ever touches its own LDS column, so
// the walk needs no barrier; the weights are staged into LDS once per workgroup and read with wave-uniform addresses.
//
//   forward   per layer the thread needs its input [C_in][L_in], one conv line [L_out] and its output [C_out][k]; input and
//             output sit at opposite ends of one region of max_l (in + line + out) slots, swapping ends from layer to layer,
//             so a layer's output is the next one's input where it lies (151 slots = 38.6 KB per wave at F = 26, [4,4,2] /
//             [6,5,3]).
//   backward  rebuilds the forward first, keeping every layer's output a_1 .. a_L (tanh' = 1 - a^2) and the selection of
//             each (layer, channel) as a 64-bit mask over the conv line; the input itself is read from global memory where
//             layer 0 needs it (once for the conv, once for dW) instead of taking LDS.  Then, last layer first and channel by
//             channel: the gradient of the kept positions is scattered into the conv line (dy), db and dW[co, ci, j] =
//             sum_p dy[p] in[ci][p + j - (kh - 1)] are reduced over the wave (a fixed butterfly) and added by lane 0 to the
//             workgroup's accumulator in LDS, and the input gradient g_l[ci][q] += sum_j w[co, ci, j] dy[q + kh - 1 - j]
//             accumulates in LDS; g_l and g_{l+1} share one region from opposite ends.  g_0 leaves as dx.  At the end of its
//             walk the workgroup writes its accumulator as ITS partial into the workspace; a finishing launch sums the
//             partials in workgroup order.  No floating-point atomics: bit-identical from run to run; the workspace is
//             CCPM_BWD_BLOCKS partials whatever the batch.
//
// Selection.  Position i of a line is kept iff rank_i = #{j : y_j > y_i or (y_j == y_i and j < i)} < k: the k largest in
// their original order, exact ties to the lower index.  L_out^2 compares, four values of i per pass over the line.
#include "common.h"

#define CCPM_T 64            // threads per workgroup = columns per tile (one wave)
#define CCPM_MAXL 3          // layers
#define CCPM_MAXC 4          // channels of a layer
#define CCPM_MAXKH 8         // kernel height
#define CCPM_MAXLEN 64       // conv line length (the selection mask is 64 bits)
#define CCPM_FWD_BLOCKS 2048 // grid caps (grid-stride over the column tiles beyond)
#define CCPM_BWD_BLOCKS 512  // = partials in the workspace
#define CCPM_LDS_FLOATS 36864  // 144 KiB of the CU's 160

struct CcpmArgs {
    const float *w[CCPM_MAXL], *b[CCPM_MAXL];
    int nl, F, D, np;  // np: parameters of the stack (every W, then b, layer by layer: woff / boff)
    int cin[CCPM_MAXL], cout[CCPM_MAXL], kh[CCPM_MAXL], k[CCPM_MAXL], lin[CCPM_MAXL], lout[CCPM_MAXL];
    int woff[CCPM_MAXL], boff[CCPM_MAXL];
    // per-thread slots.  forward: input / line / output of layer l; backward: a_{l+1}, masks of layer l, g_l (l = 0 .. nl)
    int in_off[CCPM_MAXL], line_off[CCPM_MAXL], out_off[CCPM_MAXL];
    int act_off[CCPM_MAXL], mask_off[CCPM_MAXL], g_off[CCPM_MAXL + 1], bline_off;
    int wpad;            // floats of LDS ahead of the per-thread slots (weights; backward: + the accumulator)
    int fwd_slots, bwd_slots;
};

// fills the geometry; false outside the supported range
static bool ccpm_geom(int F, int D, int nl, const int *channels, const int *heights, const int *ks, CcpmArgs *a) {
    if (nl < 1 || nl > CCPM_MAXL || F < 1 || F > CCPM_MAXLEN || D < 1 || D > 65536 || !channels || !heights || !ks) return false;
    a->nl = nl, a->F = F, a->D = D;
    int lin = F, cin = 1, np = 0, fwd = 0, acts = 0, masks = 0, maxline = 0, gmax = 0;
    for (int l = 0; l < nl; ++l) {
        const int co = channels[l], kh = heights[l], k = ks[l];
        if (co < 1 || co > CCPM_MAXC || kh < 1 || kh > CCPM_MAXKH || k < 1) return false;
        const int lout = lin + kh - 1;
        if (lout > CCPM_MAXLEN || lout < k) return false;  // (lout < k: the reference's topk raises)
        a->cin[l] = cin, a->cout[l] = co, a->kh[l] = kh, a->k[l] = k, a->lin[l] = lin, a->lout[l] = lout;
        a->woff[l] = np, np += co * cin * kh;
        a->boff[l] = np, np += co;
        const int in = cin * lin, out = co * k;
        if (in + lout + out > fwd) fwd = in + lout + out;
        if (in + out > gmax) gmax = in + out;
        if (lout > maxline) maxline = lout;
        acts += out, masks += 2 * co;
        lin = k, cin = co;
    }
    a->np = np;
    a->fwd_slots = fwd;
    lin = F, cin = 1;
    int act = 0, mask = acts;
    for (int l = 0; l < nl; ++l) {
        const int in = cin * lin, out = a->cout[l] * a->k[l];
        // forward: even layers read from the low end and write to the high end, odd layers the other way round
        a->in_off[l] = (l & 1) ? fwd - in : 0;
        a->out_off[l] = (l & 1) ? 0 : fwd - out;
        a->line_off[l] = (l & 1) ? out : in;
        a->act_off[l] = act, act += out;
        a->mask_off[l] = mask, mask += 2 * a->cout[l];
        lin = a->k[l], cin = a->cout[l];
    }
    a->bline_off = acts + masks;
    const int g0 = acts + masks + maxline;
    for (int l = 0; l <= nl; ++l) {
        const int size = l == 0 ? F : a->cout[l - 1] * a->k[l - 1];
        a->g_off[l] = (l & 1) ? g0 + gmax - size : g0;
    }
    a->bwd_slots = g0 + gmax;
    a->wpad = rp_round_up(np, 64);
    return a->wpad + CCPM_T * a->fwd_slots <= CCPM_LDS_FLOATS && 2 * a->wpad + CCPM_T * a->bwd_slots <= CCPM_LDS_FLOATS;
}

struct CcpmLdsIn {  // a layer's input in the thread's LDS slots
    const float *p;
    int lin;
    __device__ __forceinline__ float operator()(int ci, int q) const { return p[(ci * lin + q) * CCPM_T]; }
};
struct CcpmGlobalIn {  // layer 0's single input channel in the caller's rows: x[b, q, d]
    const float *p;
    int D;
    __device__ __forceinline__ float operator()(int, int q) const { return p[(int64_t)q * D]; }
};

// the conv line of one output channel: line[p] = bias + sum_{ci, j} w[ci, j] in[ci][p + j - (kh - 1)] over the zero padding
template <class In>
__device__ __forceinline__ void ccpm_conv_line(const float *__restrict__ w, float bias, In in, int cin, int kh, int lin,
                                               int lout, float *__restrict__ line) {
    for (int p = 0; p < lout; ++p) {
        const int jlo = kh - 1 - p > 0 ? kh - 1 - p : 0, jhi = lin + kh - 1 - p < kh ? lin + kh - 1 - p : kh;
        float acc = bias;
        for (int ci = 0; ci < cin; ++ci)
            for (int j = jlo; j < jhi; ++j) acc += w[ci * kh + j] * in(ci, p + j - (kh - 1));
        line[p * CCPM_T] = acc;
    }
}

// keeps the k largest of line[0 .. lout) in their order (ties to the lower index): tanh of them to out[0 .. k), -> the mask
__device__ __forceinline__ uint64_t ccpm_select(const float *__restrict__ line, int lout, int k, float *__restrict__ out) {
    uint64_t mask = 0;
    int cnt = 0;
    for (int i0 = 0; i0 < lout; i0 += 4) {
        float y[4];
        int r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            y[u] = line[(i0 + u < lout ? i0 + u : lout - 1) * CCPM_T];
            r[u] = 0;
        }
        for (int j = 0; j < lout; ++j) {
            const float yj = line[j * CCPM_T];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] += (yj > y[u] || (yj == y[u] && j < i0 + u)) ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < lout && r[u] < k && cnt < k) {  // (cnt < k: only NaNs could ask for more than k slots)
                out[cnt * CCPM_T] = tanhf(y[u]);
                mask |= 1ull << (i0 + u);
                ++cnt;
            }
        }
    }
    return mask;
}

__device__ __forceinline__ void ccpm_stage_weights(const CcpmArgs &a, float *__restrict__ ws) {
    for (int l = 0; l < a.nl; ++l) {
        const int nw = a.cout[l] * a.cin[l] * a.kh[l];
        for (int i = threadIdx.x; i < nw; i += CCPM_T) ws[a.woff[l] + i] = a.w[l][i];
        for (int i = threadIdx.x; i < a.cout[l]; i += CCPM_T) ws[a.boff[l] + i] = a.b[l][i];
    }
}

__global__ __launch_bounds__(CCPM_T) void ccpm_fwd_kernel(const float *__restrict__ x, int64_t ldx, float *__restrict__ out,
                                                          int64_t ldo, int64_t ncols, CcpmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ccpm_lds[];
    float *ws = ccpm_lds, *reg = ccpm_lds + a.wpad + threadIdx.x;
    ccpm_stage_weights(a, ws);
    __syncthreads();
    const int64_t ntiles = (ncols + CCPM_T - 1) / CCPM_T;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t col = tile * CCPM_T + threadIdx.x;
        if (col >= ncols) continue;
        const int64_t b = col / a.D;
        const int d = (int)(col - b * a.D);
        const float *xc = x + b * ldx + d;
        for (int f = 0; f < a.F; ++f) reg[(a.in_off[0] + f) * CCPM_T] = xc[(int64_t)f * a.D];
        for (int l = 0; l < a.nl; ++l) {
            const int cin = a.cin[l], kh = a.kh[l], k = a.k[l], lin = a.lin[l], lout = a.lout[l];
            const CcpmLdsIn in{reg + a.in_off[l] * CCPM_T, lin};
            float *line = reg + a.line_off[l] * CCPM_T;
            for (int co = 0; co < a.cout[l]; ++co) {
                ccpm_conv_line(ws + a.woff[l] + co * cin * kh, ws[a.boff[l] + co], in, cin, kh, lin, lout, line);
                (void)ccpm_select(line, lout, k, reg + (a.out_off[l] + co * k) * CCPM_T);
            }
        }
        const int last = a.nl - 1, n = a.cout[last] * a.k[last];  // flatten(conv_out, 1): c (k D) + j D + d
        const float *res = reg + a.out_off[last] * CCPM_T;
        float *oc = out + b * ldo + d;
        for (int i = 0; i < n; ++i) oc[(int64_t)i * a.D] = res[i * CCPM_T];
    }
}

template <class In>
__device__ __forceinline__ void ccpm_bwd_channel(const float *__restrict__ w, In in, int cin, int kh, int lin, int lout,
                                                 const float *__restrict__ line, float *__restrict__ accw,
                                                 float *__restrict__ accb, float *__restrict__ gin, bool first) {
    float s = 0.f;
    for (int p = 0; p < lout; ++p) s += line[p * CCPM_T];
    s = rp_lane_sum_up<CCPM_T>(s);
    if (threadIdx.x == 0) *accb += s;
    for (int ci = 0; ci < cin; ++ci) {
        for (int j = 0; j < kh; ++j) {  // dW[ci, j]: positions p with 0 <= p + j - (kh - 1) < lin
            const int plo = kh - 1 - j, phi = lin + kh - 1 - j < lout ? lin + kh - 1 - j : lout;
            float sw = 0.f;
            for (int p = plo; p < phi; ++p) sw += line[p * CCPM_T] * in(ci, p + j - (kh - 1));
            sw = rp_lane_sum_up<CCPM_T>(sw);
            if (threadIdx.x == 0) accw[ci * kh + j] += sw;
        }
        for (int q = 0; q < lin; ++q) {  // (q + kh - 1 - j always lies inside the line)
            float g = 0.f;
            for (int j = 0; j < kh; ++j) g += w[ci * kh + j] * line[(q + kh - 1 - j) * CCPM_T];
            float *dst = gin + (ci * lin + q) * CCPM_T;
            *dst = first ? g : *dst + g;
        }
    }
}

__global__ __launch_bounds__(CCPM_T) void ccpm_bwd_kernel(const float *__restrict__ dout, int64_t lddo,
                                                          const float *__restrict__ x, int64_t ldx, float *__restrict__ dx,
                                                          int64_t lddx, float *__restrict__ part, int64_t ncols,
                                                          CcpmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ccpm_lds[];
    float *ws = ccpm_lds, *acc = ccpm_lds + a.wpad, *reg = ccpm_lds + 2 * a.wpad + threadIdx.x;
    ccpm_stage_weights(a, ws);
    for (int i = threadIdx.x; i < a.np; i += CCPM_T) acc[i] = 0.f;
    __syncthreads();
    float *line = reg + a.bline_off * CCPM_T;
    const int64_t ntiles = (ncols + CCPM_T - 1) / CCPM_T;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // a lane beyond the last column repeats that column with a zero upstream gradient: it takes part in the wave's sums
        // (adding exact zeros) and stores nothing
        const int64_t own = tile * CCPM_T + threadIdx.x;
        const bool live = own < ncols;
        const int64_t col = live ? own : ncols - 1;
        const int64_t b = col / a.D;
        const int d = (int)(col - b * a.D);
        const CcpmGlobalIn xin{x + b * ldx + d, a.D};
        for (int l = 0; l < a.nl; ++l) {  // the forward again: a_{l+1} and the masks stay
            const int cin = a.cin[l], kh = a.kh[l], k = a.k[l], lin = a.lin[l], lout = a.lout[l];
            for (int co = 0; co < a.cout[l]; ++co) {
                const float *w = ws + a.woff[l] + co * cin * kh;
                if (l == 0) ccpm_conv_line(w, ws[a.boff[l] + co], xin, cin, kh, lin, lout, line);
                else ccpm_conv_line(w, ws[a.boff[l] + co], CcpmLdsIn{reg + a.act_off[l - 1] * CCPM_T, lin}, cin, kh, lin, lout, line);
                const uint64_t m = ccpm_select(line, lout, k, reg + (a.act_off[l] + co * k) * CCPM_T);
                reg[(a.mask_off[l] + 2 * co) * CCPM_T] = __uint_as_float((uint32_t)m);
                reg[(a.mask_off[l] + 2 * co + 1) * CCPM_T] = __uint_as_float((uint32_t)(m >> 32));
            }
        }
        {
            const int last = a.nl - 1, n = a.cout[last] * a.k[last];
            const float *gc = dout + b * lddo + d;
            float *g = reg + a.g_off[a.nl] * CCPM_T;
            for (int i = 0; i < n; ++i) g[i * CCPM_T] = live ? gc[(int64_t)i * a.D] : 0.f;
        }
        for (int l = a.nl - 1; l >= 0; --l) {
            const int cin = a.cin[l], kh = a.kh[l], k = a.k[l], lin = a.lin[l], lout = a.lout[l];
            const float *gout = reg + a.g_off[l + 1] * CCPM_T, *aout = reg + a.act_off[l] * CCPM_T;
            float *gin = reg + a.g_off[l] * CCPM_T;
            for (int co = 0; co < a.cout[l]; ++co) {
                const uint64_t m = (uint64_t)__float_as_uint(reg[(a.mask_off[l] + 2 * co) * CCPM_T]) |
                                   ((uint64_t)__float_as_uint(reg[(a.mask_off[l] + 2 * co + 1) * CCPM_T]) << 32);
                int cnt = 0;
                for (int p = 0; p < lout; ++p) {  // dy: the kept positions take their slot's gradient through tanh'
                    float dy = 0.f;
                    if (((m >> p) & 1) != 0 && cnt < k) {
                        const float y = aout[(co * k + cnt) * CCPM_T];
                        dy = gout[(co * k + cnt) * CCPM_T] * (1.f - y * y);
                        ++cnt;
                    }
                    line[p * CCPM_T] = dy;
                }
                const float *w = ws + a.woff[l] + co * cin * kh;
                float *accw = acc + a.woff[l] + co * cin * kh, *accb = acc + a.boff[l] + co;
                if (l == 0) ccpm_bwd_channel(w, xin, cin, kh, lin, lout, line, accw, accb, gin, co == 0);
                else ccpm_bwd_channel(w, CcpmLdsIn{reg + a.act_off[l - 1] * CCPM_T, lin}, cin, kh, lin, lout, line, accw, accb, gin, co == 0);
            }
        }
        if (live) {
            const float *g0 = reg + a.g_off[0] * CCPM_T;
            float *dc = dx + b * lddx + d;
            for (int f = 0; f < a.F; ++f) dc[(int64_t)f * a.D] = g0[f * CCPM_T];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.np; i += CCPM_T) part[(int64_t)blockIdx.x * a.np + i] = acc[i];
}

struct CcpmGradPtrs {
    float *dw[CCPM_MAXL], *db[CCPM_MAXL];
};

// one thread per parameter: its partials summed in workgroup order
__global__ __launch_bounds__(256) void ccpm_bwd_finish_kernel(const float *__restrict__ part, int nblk, CcpmGradPtrs g,
                                                              CcpmArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.np) return;
    float s = 0.f;
    for (int blk = 0; blk < nblk; ++blk) s += part[(int64_t)blk * a.np + i];
    for (int l = 0; l < a.nl; ++l) {
        if (i >= a.woff[l] && i < a.boff[l]) g.dw[l][i - a.woff[l]] = s;
        else if (i >= a.boff[l] && i < a.boff[l] + a.cout[l]) g.db[l][i - a.boff[l]] = s;
    }
}

extern "C" int rp_ccpm_fits(int F, int D, int n_layers, const int *channels, const int *heights, const int *ks) {
    CcpmArgs a{};
    return ccpm_geom(F, D, n_layers, channels, heights, ks, &a) ? 1 : 0;
}

extern "C" int rp_ccpm_fwd(const float *x, int64_t ldx, const float *const *W, const float *const *bias, float *out,
                           int64_t ldo, int F, int D, int n_layers, const int *channels, const int *heights, const int *ks,
                           int64_t B, rp_stream_t stream) {
    RP_REQUIRE(x && W && bias && out && channels && heights && ks, "ccpm_fwd: null pointer");
    RP_REQUIRE(F >= 1 && D >= 1 && n_layers >= 1 && B >= 0, "ccpm_fwd: bad F / D / n_layers / B");
    CcpmArgs a{};
    if (!ccpm_geom(F, D, n_layers, channels, heights, ks, &a))
        return rp_fail(RP_ERR_UNSUPPORTED, "ccpm_fwd: F=%d D=%d with %d layers outside rp_ccpm_fits", F, D, n_layers);
    const int last = n_layers - 1;
    RP_REQUIRE(ldx >= (int64_t)F * D && ldo >= (int64_t)a.cout[last] * a.k[last] * D, "ccpm_fwd: leading dimension too small");
    for (int l = 0; l < n_layers; ++l) {
        RP_REQUIRE(W[l] && bias[l], "ccpm_fwd: null pointer (layer %d)", l);
        a.w[l] = W[l], a.b[l] = bias[l];
    }
    if (B == 0) return RP_OK;
    const int64_t ncols = B * D;
    int64_t blocks = rp_cdiv(ncols, CCPM_T);
    if (blocks > CCPM_FWD_BLOCKS) blocks = CCPM_FWD_BLOCKS;
    const size_t lds = (size_t)(a.wpad + CCPM_T * a.fwd_slots) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ccpm_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(ccpm_fwd_kernel, dim3((unsigned)blocks), dim3(CCPM_T), (unsigned)lds, s, x, ldx, out, ldo, ncols, a);
    RP_LAUNCH_CHECK("ccpm_fwd");
    return RP_OK;
}

extern "C" int rp_ccpm_bwd_workspace_bytes(int n_layers, const int *channels, const int *heights, size_t *bytes) {
    RP_REQUIRE(bytes && channels && heights && n_layers >= 1 && n_layers <= CCPM_MAXL, "ccpm_bwd_workspace_bytes: bad argument");
    size_t np = 0;
    int cin = 1;
    for (int l = 0; l < n_layers; ++l) {
        RP_REQUIRE(channels[l] >= 1 && heights[l] >= 1, "ccpm_bwd_workspace_bytes: bad layer %d", l);
        np += (size_t)channels[l] * cin * heights[l] + channels[l];
        cin = channels[l];
    }
    *bytes = (size_t)CCPM_BWD_BLOCKS * np * sizeof(float) + 256;
    return RP_OK;
}

extern "C" int rp_ccpm_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *const *W,
                           const float *const *bias, float *dx, int64_t lddx, float *const *dW, float *const *db, int F, int D,
                           int n_layers, const int *channels, const int *heights, const int *ks, int64_t B, void *workspace,
                           size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(dout && x && W && bias && dx && dW && db && channels && heights && ks && workspace, "ccpm_bwd: null pointer");
    RP_REQUIRE(F >= 1 && D >= 1 && n_layers >= 1 && B >= 1, "ccpm_bwd: bad F / D / n_layers / B");
    CcpmArgs a{};
    if (!ccpm_geom(F, D, n_layers, channels, heights, ks, &a))
        return rp_fail(RP_ERR_UNSUPPORTED, "ccpm_bwd: F=%d D=%d with %d layers outside rp_ccpm_fits", F, D, n_layers);
    const int last = n_layers - 1;
    RP_REQUIRE(ldx >= (int64_t)F * D && lddx >= (int64_t)F * D && lddo >= (int64_t)a.cout[last] * a.k[last] * D,
               "ccpm_bwd: leading dimension too small");
    CcpmGradPtrs g;
    for (int l = 0; l < n_layers; ++l) {
        RP_REQUIRE(W[l] && bias[l] && dW[l] && db[l], "ccpm_bwd: null pointer (layer %d)", l);
        a.w[l] = W[l], a.b[l] = bias[l], g.dw[l] = dW[l], g.db[l] = db[l];
    }
    size_t need = 0;
    rp_ccpm_bwd_workspace_bytes(n_layers, channels, heights, &need);
    RP_REQUIRE(workspace_bytes >= need, "ccpm_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    float *part = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    const int64_t ncols = B * D;
    int64_t blocks = rp_cdiv(ncols, CCPM_T);
    if (blocks > CCPM_BWD_BLOCKS) blocks = CCPM_BWD_BLOCKS;
    const size_t lds = (size_t)(2 * a.wpad + CCPM_T * a.bwd_slots) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ccpm_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(ccpm_bwd_kernel, dim3((unsigned)blocks), dim3(CCPM_T), (unsigned)lds, s, dout, lddo, x, ldx, dx, lddx,
                       part, ncols, a);
    RP_LAUNCH_CHECK("ccpm_bwd");
    hipLaunchKernelGGL(ccpm_bwd_finish_kernel, dim3((unsigned)rp_cdiv(a.np, 256)), dim3(256), 0, s, part, (int)blocks, g, a);
    RP_LAUNCH_CHECK("ccpm_bwd (finish)");
    return RP_OK;
}
