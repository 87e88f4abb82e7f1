// Multi-layer GRU recurrence of the sequence-recall models GRU4Rec and NARM, gfx950 — replaces nn.GRU(batch_first=True)
// (rec_pangu/models/layers/sequence.py:231-251 packed by length, rec_pangu/models/sequence/narm.py:21,49 over all L
// positions) and its autograd, plus NARM's attention readout (narm.py:52-61).
//
// torch's gates, order r, z, n:   r = s(Wir x + bir + Whr h + bhr)   z = s(Wiz x + biz + Whz h + bhz)
//                                 n = tanh(Win x + bin + r (Whn h + bhn))        h' = (1 - z) n + z h,      h_0 = 0
//
// ONE launch per layer and direction walks all L steps.  A workgroup owns GRU_TB = 32 batch rows; wave w owns the hidden
// columns [32 w, 32 w + 32) of all three gates, so the gate arithmetic needs no exchange: four 32 x 32 accumulator tiles per
// wave (r and z take x's and h's products into one tile, n keeps them apart) on the exact-fp32 matrix core
// (v_mfma_f32_32x32x2_f32: an fp32 FMA chain, so the L-fold feedback carries fp32 rounding only).  h stays in the wave's
// registers in the accumulator layout from step to step and goes through LDS once per step as the next product's A operand;
// its only trip to global memory is the store of H_all[b, t] the backward needs.  Weights are read from zero-padded copies
// [3 Hp][Kp] (Hp, Kp: H, in rounded up to 32; one small launch per call): the forward keeps them in LDS for the whole walk
// when x tile + h tile + both matrices fit the CU's 160 KiB (in = H = 64: 119 KiB), otherwise they stay in L2.
//
// Backward: walks t downwards with dh in registers, recomputes the gates from x_t and h_{t-1} = H_all[b, t - 1], multiplies
// the gate gradients by W_hh / W_ih through LDS (contraction over the 3 Hp gate columns, which span the waves) and writes
//   dgi [B, L, 3H] = (dar, daz, dan)            dghs [B, L, 3H]: slot t holds (dar, daz, dan r) of step t + 1, slot L - 1 zero
// so that dW_ih = dgi^T X and dW_hh = dghs^T H_all are two calls of the library's deterministic weight-gradient GEMM over
// the same B L rows, db_ih its column sums.  db_hh's n part (the sum over ALL steps, step 0 included) is summed per lane in
// step order into one slab per workgroup and added in workgroup order by a second launch; its r, z parts equal db_ih's.
// No floating-point atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

constexpr int GRU_TB = 32;
constexpr int GRU_MAX = 128;
constexpr size_t GRU_LDS_MAX = 160 * 1024 - 512;

// dst_i [3 Hp][Kp], dst_h [3 Hp][Hp]: zero-padded copies of W_ih [3H][in], W_hh [3H][H]
__global__ __launch_bounds__(256) void gru_pad_w_kernel(const float *__restrict__ wi, const float *__restrict__ wh, int in,
                                                        int H, int Kp, int Hp, float *__restrict__ di,
                                                        float *__restrict__ dh) {
    const int ni = 3 * Hp * Kp, nh = 3 * Hp * Hp;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < ni + nh; idx += gridDim.x * 256) {
        const bool first = idx < ni;
        const int e = first ? idx : idx - ni, ld = first ? Kp : Hp, K = first ? in : H;
        const int k = e % ld, rp = e / ld, g = rp / Hp, j = rp % Hp;
        const float v = (j < H && k < K) ? (first ? wi : wh)[(int64_t)(g * H + j) * K + k] : 0.f;
        (first ? di : dh)[e] = v;
    }
}

// x_t of the workgroup's 32 rows -> xs [32][ldx], zero beyond `in` and beyond B; id mode gathers E's rows (an id outside
// [0, V) raises the flag and reads row 0, as rp_hist_mean_fwd does) and, when xg is given, leaves the gathered row there
__device__ __forceinline__ void gru_stage_x(const int64_t *__restrict__ ids, const float *__restrict__ E, int64_t V,
                                            const float *__restrict__ X, int64_t B, int64_t L, int in, int Kp, int ldx,
                                            int64_t b0, int64_t t, float *xs, float *__restrict__ xg,
                                            int32_t *__restrict__ err_flag) {
    for (int idx = threadIdx.x; idx < GRU_TB * Kp; idx += blockDim.x) {
        const int row = idx / Kp, k = idx % Kp;
        const int64_t b = b0 + row;
        float v = 0.f;
        if (b < B && k < in) {
            if (ids != nullptr) {
                int64_t id = ids[b * L + t];
                if (id < 0 || id >= V) {
                    if (err_flag != nullptr) *err_flag = 1;
                    id = 0;
                }
                v = E[id * in + k];
                if (xg != nullptr) xg[(b * L + t) * in + k] = v;
            } else {
                v = X[(b * L + t) * in + k];
            }
        }
        xs[row * ldx + k] = v;
    }
}

// the four gate tiles of one step: ar / az take x's and h's products, ani / anh keep n's apart
__device__ __forceinline__ void gru_gate_tiles(const float *xs, int ldx, const float *hs, int ldh, const float *wi, int ldwi,
                                               const float *wh, int ldwh, int Kp, int Hp, int i, int h, int j, f32x16 &ar,
                                               f32x16 &az, f32x16 &ani, f32x16 &anh) {
    for (int kq = 0; kq < Kp / 8; ++kq) {
        const int k = kq * 8 + 4 * h;
        const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&xs[i * ldx + k]);
        const f32x4 wr = *reinterpret_cast<const f32x4 *>(&wi[(int64_t)j * ldwi + k]);
        const f32x4 wz = *reinterpret_cast<const f32x4 *>(&wi[(int64_t)(Hp + j) * ldwi + k]);
        const f32x4 wn = *reinterpret_cast<const f32x4 *>(&wi[(int64_t)(2 * Hp + j) * ldwi + k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ar = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wr[e], ar, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wz[e], az, 0, 0, 0);
            ani = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wn[e], ani, 0, 0, 0);
        }
    }
    for (int kq = 0; kq < Hp / 8; ++kq) {
        const int k = kq * 8 + 4 * h;
        const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&hs[i * ldh + k]);
        const f32x4 wr = *reinterpret_cast<const f32x4 *>(&wh[(int64_t)j * ldwh + k]);
        const f32x4 wz = *reinterpret_cast<const f32x4 *>(&wh[(int64_t)(Hp + j) * ldwh + k]);
        const f32x4 wn = *reinterpret_cast<const f32x4 *>(&wh[(int64_t)(2 * Hp + j) * ldwh + k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ar = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wr[e], ar, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wz[e], az, 0, 0, 0);
            anh = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], wn[e], anh, 0, 0, 0);
        }
    }
}

struct GruBias {
    float r, z, in, hn;
};

__device__ __forceinline__ GruBias gru_bias(const float *__restrict__ bih, const float *__restrict__ bhh, int H, int j) {
    GruBias b{0.f, 0.f, 0.f, 0.f};
    if (j < H) {
        if (bih != nullptr) b.r += bih[j], b.z += bih[H + j], b.in = bih[2 * H + j];
        if (bhh != nullptr) b.r += bhh[j], b.z += bhh[H + j], b.hn = bhh[2 * H + j];
    }
    return b;
}

// block of 64 * (Hp / 32) threads; dynamic LDS: xs [32][Kp + 4], hs [32][Hp + 4] (+ both padded matrices when WLDS)
template <bool WLDS>
__global__ __launch_bounds__(256) void gru_fwd_kernel(const int64_t *__restrict__ ids, const float *__restrict__ E, int64_t V,
                                                      const float *__restrict__ X, int64_t B, int64_t L, int in, int H, int Kp,
                                                      int Hp, const float *__restrict__ Wi, const float *__restrict__ Wh,
                                                      const float *__restrict__ bih, const float *__restrict__ bhh,
                                                      const int32_t *__restrict__ steps, const int32_t *__restrict__ last,
                                                      float *__restrict__ H_all, float *__restrict__ h_last,
                                                      int32_t *__restrict__ err_flag) {
    extern __shared__ __attribute__((aligned(16))) float gru_lds[];
    __shared__ int s_tmax;
    const int ldx = Kp + 4, ldh = Hp + 4;
    float *xs = gru_lds, *hs = xs + GRU_TB * ldx, *wis = hs + GRU_TB * ldh, *whs = wis + 3 * Hp * ldx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5, j = 32 * w + i;
    const int64_t b0 = (int64_t)blockIdx.x * GRU_TB;
    if (WLDS) {
        for (int idx = tid; idx < 3 * Hp * Kp; idx += blockDim.x) wis[(idx / Kp) * ldx + idx % Kp] = Wi[idx];
        for (int idx = tid; idx < 3 * Hp * Hp; idx += blockDim.x) whs[(idx / Hp) * ldh + idx % Hp] = Wh[idx];
    }
    for (int idx = tid; idx < GRU_TB * ldh; idx += blockDim.x) hs[idx] = 0.f;
    if (tid == 0) s_tmax = 0;
    const float *wi = WLDS ? wis : Wi, *wh = WLDS ? whs : Wh;
    const int ldwi = WLDS ? ldx : Kp, ldwh = WLDS ? ldh : Hp;
    const GruBias bias = gru_bias(bih, bhh, H, j);
    int st[16], la[16], mine = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t b = b0 + rp_mfma32_row(r, h);
        int s = b < B ? steps[b] : 0;
        s = s < 0 ? 0 : (s > L ? (int)L : s);
        st[r] = s;
        la[r] = b < B ? last[b] : -1;
        mine = s > mine ? s : mine;
        if (b < B && j < H) h_last[b * H + j] = 0.f;  // (rewritten by this very thread at t == last[b])
    }
    __syncthreads();
    atomicMax(&s_tmax, mine);
    __syncthreads();
    const int tmax = s_tmax;
    float hreg[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) hreg[r] = 0.f;

    for (int64_t t = 0; t < L; ++t) {
        const bool live = t < tmax;  // (uniform over the workgroup)
        if (live) gru_stage_x(ids, E, V, X, B, L, in, Kp, ldx, b0, t, xs, nullptr, err_flag);
        __syncthreads();
        f32x16 ar = {0}, az = {0}, ani = {0}, anh = {0};
        if (live) gru_gate_tiles(xs, ldx, hs, ldh, wi, ldwi, wh, ldwh, Kp, Hp, i, h, j, ar, az, ani, anh);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rp_mfma32_row(r, h);
            const int64_t b = b0 + row;
            const bool active = t < st[r];
            float out = 0.f;
            if (active) {
                const float rr = rp_sigmoid(ar[r] + bias.r), zz = rp_sigmoid(az[r] + bias.z);
                const float nn = tanhf(ani[r] + bias.in + rr * (anh[r] + bias.hn));
                out = hreg[r] = (1.f - zz) * nn + zz * hreg[r];
                hs[row * ldh + j] = out;
            }
            if (b < B && j < H) {
                H_all[(b * L + t) * H + j] = out;
                if (active && t == la[r]) h_last[b * H + j] = out;
            }
        }
    }
}

// block of 64 * (Hp / 32) threads; dynamic LDS: xs [32][Kp + 4], hs [32][Hp + 4], gis / ghs [32][3 Hp + 4]
__global__ __launch_bounds__(256) void gru_bwd_kernel(const int64_t *__restrict__ ids, const float *__restrict__ E, int64_t V,
                                                      const float *__restrict__ X, int64_t B, int64_t L, int in, int H, int Kp,
                                                      int Hp, const float *__restrict__ Wi, const float *__restrict__ Wh,
                                                      const float *__restrict__ bih, const float *__restrict__ bhh,
                                                      const int32_t *__restrict__ steps, const int32_t *__restrict__ last,
                                                      const float *__restrict__ H_all, const float *__restrict__ dH_all,
                                                      const float *__restrict__ dh_last, float *__restrict__ xg,
                                                      float *__restrict__ dX, float *__restrict__ dgi,
                                                      float *__restrict__ dghs, float *__restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) float gru_lds[];
    const int ldx = Kp + 4, ldh = Hp + 4, ldg = 3 * Hp + 4;
    float *xs = gru_lds, *hs = xs + GRU_TB * ldx, *gis = hs + GRU_TB * ldh, *ghs = gis + GRU_TB * ldg;
    const int tid = threadIdx.x, w = tid >> 6, nw = blockDim.x >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int j = 32 * w + i;
    const int64_t b0 = (int64_t)blockIdx.x * GRU_TB;
    const GruBias bias = gru_bias(bih, bhh, H, j);
    const int H3 = 3 * H;
    int st[16], la[16];
    float dhc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t b = b0 + rp_mfma32_row(r, h);
        int s = b < B ? steps[b] : 0;
        st[r] = s < 0 ? 0 : (s > L ? (int)L : s);
        la[r] = b < B ? last[b] : -1;
        dhc[r] = 0.f;
        if (b < B && j < H) {  // (slot L - 1 of the shifted buffer pairs with h_{L-1}: no step follows it)
            float *o = dghs + (b * L + L - 1) * H3 + j;
            o[0] = 0.f, o[H] = 0.f, o[2 * H] = 0.f;
        }
    }
    float dbn = 0.f;

    for (int64_t t = L - 1; t >= 0; --t) {
        gru_stage_x(ids, E, V, X, B, L, in, Kp, ldx, b0, t, xs, xg, nullptr);
        for (int idx = tid; idx < GRU_TB * Hp; idx += blockDim.x) {
            const int row = idx / Hp, k = idx % Hp;
            const int64_t b = b0 + row;
            hs[row * ldh + k] = (t > 0 && b < B && k < H) ? H_all[(b * L + t - 1) * H + k] : 0.f;
        }
        __syncthreads();
        f32x16 ar = {0}, az = {0}, ani = {0}, anh = {0};
        gru_gate_tiles(xs, ldx, hs, ldh, Wi, Kp, Wh, Hp, Kp, Hp, i, h, j, ar, az, ani, anh);
        float keep[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rp_mfma32_row(r, h);
            const int64_t b = b0 + row;
            const bool mine = b < B && j < H, active = mine && t < st[r];
            float dar = 0.f, daz = 0.f, dan = 0.f, dhn = 0.f;
            keep[r] = 0.f;
            if (active) {
                float dh = dhc[r];
                if (dH_all != nullptr) dh += dH_all[(b * L + t) * H + j];
                if (dh_last != nullptr && t == la[r]) dh += dh_last[b * H + j];
                const float hp = hs[row * ldh + j];
                const float rr = rp_sigmoid(ar[r] + bias.r), zz = rp_sigmoid(az[r] + bias.z);
                const float ghn = anh[r] + bias.hn;
                const float nn = tanhf(ani[r] + bias.in + rr * ghn);
                dan = dh * (1.f - zz) * (1.f - nn * nn);
                daz = dh * (hp - nn) * zz * (1.f - zz);
                dar = dan * ghn * rr * (1.f - rr);
                dhn = dan * rr;
                keep[r] = dh * zz;
            }
            gis[row * ldg + j] = dar, gis[row * ldg + Hp + j] = daz, gis[row * ldg + 2 * Hp + j] = dan;
            ghs[row * ldg + j] = dar, ghs[row * ldg + Hp + j] = daz, ghs[row * ldg + 2 * Hp + j] = dhn;
            dbn += dhn;
            if (mine) {
                float *o = dgi + (b * L + t) * H3 + j;
                o[0] = dar, o[H] = daz, o[2 * H] = dan;
                if (t > 0) {
                    float *p = dghs + (b * L + t - 1) * H3 + j;
                    p[0] = dar, p[H] = daz, p[2 * H] = dhn;
                }
            }
        }
        __syncthreads();
        {  // dh_{t-1} = dh z + dgh W_hh: this wave's 32 hidden columns, contraction over the 3 Hp gate columns
            f32x16 acc = {0};
            for (int kq = 0; kq < 3 * Hp / 8; ++kq) {
                const int k = kq * 8 + 4 * h;
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&ghs[i * ldg + k]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], Wh[(int64_t)(k + e) * Hp + j], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) dhc[r] = keep[r] + acc[r];
        }
        if (dX != nullptr) {  // dx_t = dgi W_ih, 32 input columns per tile
            for (int c = w; c < Kp / 32; c += nw) {
                const int col = 32 * c + i;
                f32x16 acc = {0};
                for (int kq = 0; kq < 3 * Hp / 8; ++kq) {
                    const int k = kq * 8 + 4 * h;
                    const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&gis[i * ldg + k]);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], Wi[(int64_t)(k + e) * Kp + col], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t b = b0 + rp_mfma32_row(r, h);
                    if (b < B && col < in) dX[(b * L + t) * in + col] = acc[r];
                }
            }
        }
        // (no barrier here: the next step's staging writes xs / hs, last read in front of the barrier above, and gis / ghs
        //  are rewritten only behind the next step's first barrier, which every wave reaches after its products)
    }
    if (slab != nullptr) {
        dbn += __shfl_xor(dbn, 32);
        if (h == 0 && j < H) slab[(int64_t)blockIdx.x * H + j] = dbn;
    }
}

// db_hh [3H]: the r, z parts are db_ih's (both biases sit in the same pre-activation), the n part the slabs in workgroup order
__global__ __launch_bounds__(256) void gru_bias_finish_kernel(const float *__restrict__ db_ih, const float *__restrict__ slab,
                                                              int64_t nslab, int H, float *__restrict__ db_hh) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 3 * H) return;
    if (c < 2 * H) {
        db_hh[c] = db_ih[c];
        return;
    }
    float s = 0.f;
    for (int64_t q = 0; q < nslab; ++q) s += slab[q * H + (c - 2 * H)];
    db_hh[c] = s;
}

struct GruWs {
    size_t wi, wh, dgi, dghs, slab, xg, wgrad, wgrad_bytes, total;
};

int gru_ws(int64_t B, int64_t L, int in, int H, int ids_mode, GruWs *o) {
    const int Kp = rp_round_up(in, 32), Hp = rp_round_up(H, 32);
    size_t off = 0, wa = 0, wb = 0;
    o->wi = off, off += rp_round_up(sizeof(float) * 3 * Hp * Kp, 256);
    o->wh = off, off += rp_round_up(sizeof(float) * 3 * Hp * Hp, 256);
    o->dgi = off, off += rp_round_up(sizeof(float) * 3 * H * (size_t)B * L, 256);
    o->dghs = off, off += rp_round_up(sizeof(float) * 3 * H * (size_t)B * L, 256);
    o->slab = off, off += rp_round_up(sizeof(float) * H * (size_t)rp_cdiv(B, GRU_TB), 256);
    o->xg = off, off += ids_mode ? rp_round_up(sizeof(float) * in * (size_t)B * L, 256) : 0;
    int rc = rp_linear_wgrad_workspace_bytes(B * L, 3 * H, in, &wa);
    if (rc != RP_OK) return rc;
    rc = rp_linear_wgrad_workspace_bytes(B * L, 3 * H, H, &wb);
    if (rc != RP_OK) return rc;
    o->wgrad = off, o->wgrad_bytes = wa > wb ? wa : wb, off += rp_round_up(o->wgrad_bytes, 256);
    o->total = off;
    return RP_OK;
}

#define GRU_CHECK_DIMS(what)                                                                                         \
    RP_REQUIRE(B >= 0 && L >= 1 && in >= 1 && in <= GRU_MAX && H >= 1 && H <= GRU_MAX,                                \
               what ": need B >= 0, L >= 1 and 1 <= in, H <= %d (got B=%lld L=%lld in=%d H=%d)", GRU_MAX, (long long)B, \
               (long long)L, in, H)

}  // namespace

extern "C" int rp_gru_geometry(int *tb, int *max_h) {
    RP_REQUIRE(tb && max_h, "gru_geometry: null pointer");
    *tb = GRU_TB, *max_h = GRU_MAX;
    return RP_OK;
}

extern "C" int rp_gru_workspace_bytes(int64_t B, int64_t L, int in, int H, int ids_mode, size_t *bytes) {
    RP_REQUIRE(bytes, "gru_workspace_bytes: null pointer");
    GRU_CHECK_DIMS("gru_workspace_bytes");
    GruWs ws;
    const int rc = gru_ws(B, L, in, H, ids_mode, &ws);
    if (rc != RP_OK) return rc;
    *bytes = ws.total;
    return RP_OK;
}

extern "C" int rp_gru_fwd(const int64_t *ids, const float *E, int64_t V, const float *X, int64_t B, int64_t L, int in, int H,
                          const float *W_ih, const float *W_hh, const float *b_ih, const float *b_hh, const int32_t *steps,
                          const int32_t *last, float *H_all, float *h_last, int32_t *err_flag, void *workspace,
                          size_t workspace_bytes, rp_stream_t stream) {
    GRU_CHECK_DIMS("gru_fwd");
    RP_REQUIRE(W_ih && W_hh && steps && last && H_all && h_last && workspace, "gru_fwd: null pointer");
    RP_REQUIRE((ids != nullptr) != (X != nullptr), "gru_fwd: give either ids (+ E) or X");
    RP_REQUIRE(ids == nullptr || (E != nullptr && err_flag != nullptr && V >= 1), "gru_fwd: id mode needs E, V >= 1 and err_flag");
    GruWs ws;
    int rc = gru_ws(B, L, in, H, ids != nullptr, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "gru_fwd: workspace too small or misaligned");
    if (B == 0) return RP_OK;
    const int Kp = rp_round_up(in, 32), Hp = rp_round_up(H, 32);
    float *wi = reinterpret_cast<float *>(static_cast<char *>(workspace) + ws.wi);
    float *wh = reinterpret_cast<float *>(static_cast<char *>(workspace) + ws.wh);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gru_pad_w_kernel, dim3((unsigned)rp_cdiv(3 * Hp * (Kp + Hp), 256)), dim3(256), 0, s, W_ih, W_hh, in, H,
                       Kp, Hp, wi, wh);
    RP_LAUNCH_CHECK("gru_fwd (weights)");
    const size_t tiles = sizeof(float) * GRU_TB * (size_t)(Kp + 4 + Hp + 4);
    const size_t resident = tiles + sizeof(float) * 3 * Hp * (size_t)(Kp + 4 + Hp + 4);
    const bool wlds = resident <= GRU_LDS_MAX;
    const size_t lds = wlds ? resident : tiles;
    const dim3 grid((unsigned)rp_cdiv(B, GRU_TB)), block(64 * (Hp / 32));
    if (wlds) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_fwd_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(gru_fwd_kernel<true>, grid, block, (unsigned)lds, s, ids, E, V, X, B, L, in, H, Kp, Hp,
                           (const float *)wi, (const float *)wh, b_ih, b_hh, steps, last, H_all, h_last, err_flag);
    } else {
        hipLaunchKernelGGL(gru_fwd_kernel<false>, grid, block, (unsigned)lds, s, ids, E, V, X, B, L, in, H, Kp, Hp,
                           (const float *)wi, (const float *)wh, b_ih, b_hh, steps, last, H_all, h_last, err_flag);
    }
    RP_LAUNCH_CHECK("gru_fwd");
    return RP_OK;
}

extern "C" int rp_gru_bwd(const int64_t *ids, const float *E, int64_t V, const float *X, int64_t B, int64_t L, int in, int H,
                          const float *W_ih, const float *W_hh, const float *b_ih, const float *b_hh, const int32_t *steps,
                          const int32_t *last, const float *H_all, const float *dH_all, const float *dh_last, float *dX,
                          float *dW_ih, float *dW_hh, float *db_ih, float *db_hh, void *workspace, size_t workspace_bytes,
                          rp_stream_t stream) {
    GRU_CHECK_DIMS("gru_bwd");
    RP_REQUIRE(W_ih && W_hh && steps && last && H_all && workspace, "gru_bwd: null pointer");
    RP_REQUIRE((ids != nullptr) != (X != nullptr), "gru_bwd: give either ids (+ E) or X");
    RP_REQUIRE(ids == nullptr || (E != nullptr && V >= 1), "gru_bwd: id mode needs E and V >= 1");
    RP_REQUIRE((dW_ih != nullptr) == (dW_hh != nullptr), "gru_bwd: dW_ih and dW_hh come together");
    RP_REQUIRE((db_ih != nullptr) == (db_hh != nullptr) && (db_ih == nullptr || (b_ih != nullptr && b_hh != nullptr && dW_ih)),
               "gru_bwd: db_ih and db_hh come together, with biases and the weight gradients");
    GruWs ws;
    int rc = gru_ws(B, L, in, H, ids != nullptr, &ws);
    if (rc != RP_OK) return rc;
    RP_REQUIRE(workspace_bytes >= ws.total && rp_aligned16(workspace), "gru_bwd: workspace too small or misaligned");
    if (B == 0) return RP_OK;
    const int Kp = rp_round_up(in, 32), Hp = rp_round_up(H, 32);
    char *base = static_cast<char *>(workspace);
    float *wi = reinterpret_cast<float *>(base + ws.wi), *wh = reinterpret_cast<float *>(base + ws.wh);
    float *dgi = reinterpret_cast<float *>(base + ws.dgi), *dghs = reinterpret_cast<float *>(base + ws.dghs);
    float *slab = db_hh ? reinterpret_cast<float *>(base + ws.slab) : nullptr;
    float *xg = ids ? reinterpret_cast<float *>(base + ws.xg) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gru_pad_w_kernel, dim3((unsigned)rp_cdiv(3 * Hp * (Kp + Hp), 256)), dim3(256), 0, s, W_ih, W_hh, in, H,
                       Kp, Hp, wi, wh);
    RP_LAUNCH_CHECK("gru_bwd (weights)");
    const size_t lds = sizeof(float) * GRU_TB * (size_t)(Kp + 4 + Hp + 4 + 2 * (3 * Hp + 4));
    const int64_t nwg = rp_cdiv(B, GRU_TB);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(gru_bwd_kernel, dim3((unsigned)nwg), dim3(64 * (Hp / 32)), (unsigned)lds, s, ids, E, V, X, B, L, in, H,
                       Kp, Hp, (const float *)wi, (const float *)wh, b_ih, b_hh, steps, last, H_all, dH_all, dh_last, xg, dX,
                       dgi, dghs, slab);
    RP_LAUNCH_CHECK("gru_bwd");
    if (dW_ih == nullptr) return RP_OK;
    rc = rp_linear_wgrad(dgi, 3 * H, ids ? xg : X, in, dW_ih, in, db_ih, B * L, 3 * H, in, 0, base + ws.wgrad, ws.wgrad_bytes,
                         stream);
    if (rc != RP_OK) return rc;
    rc = rp_linear_wgrad(dghs, 3 * H, H_all, H, dW_hh, H, nullptr, B * L, 3 * H, H, 0, base + ws.wgrad, ws.wgrad_bytes, stream);
    if (rc != RP_OK) return rc;
    if (db_hh != nullptr) {
        hipLaunchKernelGGL(gru_bias_finish_kernel, dim3((unsigned)rp_cdiv(3 * H, 256)), dim3(256), 0, s, (const float *)db_ih,
                           (const float *)slab, nwg, H, db_hh);
        RP_LAUNCH_CHECK("gru_bwd (bias)");
    }
    return RP_OK;
}
