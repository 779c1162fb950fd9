// twv_wavenet_wide.hip -- WaveNet generation for residual_channels R / dilation_channels D in {32, 64, 128}, (R, D) != (32, 32).
//
// Replaces, for hccho2/Tacotron-Wavenet-Vocoder-Korean at those widths (wavenet/model.py:8-10 takes any width):
//   wavenet/model.py:41-167,215-245  (incremental network)   -> wn_wide_generate_kernel (persistent, one launch per call)
//   wavenet/mixture.py:84-114        (MoL sampler)           -> fused
//   generate.py:199-233              (per-sample host loop)  -> the kernel's step loop
//   wavenet/model.py:71-83,181-212   (gc/lc 1x1 projections) -> hoisted: wn_wide_proj_kernel
//
// Design (DESIGN.md "Wide models"): ONE workgroup of 16 waves per stream and no communication between workgroups, so there is no
// co-residency condition, no wait that another workgroup has to end, and any batch size runs.  Inside the workgroup the phases of a
// step are separated by __syncthreads() only (every thread takes every barrier: the trip counts are kernel arguments).  Weights are
// never resident: every wave streams the 64x32 tiles of its (output block, chunk) work global -> registers; the operand vectors
// (x, x[t-d], z, h1, h2), the tap-0 partial sums of all layers and the logits live in LDS; the delay lines stay in HBM.
// Arithmetic: DESIGN.md AC-1..AC-5, at K > 32 exactly the CPU checker's head/tail split (AC-1b): bit-identical results.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_layout.hpp"
#include "twv_math.hpp"
#include "twv_dev.hpp"
#include "twv_categorical.hpp"
#include "twv_wide.hpp"

using namespace twv;

int twv_fail(int code, const std::string& msg);

namespace {

constexpr int kWideThreads = 1024;
constexpr int kWideWaves = kWideThreads / 64;
constexpr int kWideLdsBytes = 160 * 1024;

// LDS map (float offsets); shared by the kernel and the host's size computation
struct WideLds {
    int o_meta;    // [192] ints: dil[64] | ring_off[64] | delay-line write position at launch[64]
    int o_ctl;     // [16]  word 0: the sample just drawn
    int o_hist;    // [64]  causal queue (scalar input): entry k = the k-th oldest of the last ifw inputs, zero beyond ifw
    int o_x;       // [128] residual vector x of the layer about to run
    int o_z;       // [128] gated output z of the current layer
    int o_h1;      // [S]   relu(sum of skips)
    int o_h2;      // [S]   relu(conv1d_1)
    int o_lg;      // [Opad] raw network outputs
    int o_xold;    // [NL][R]  x_l[t - d_l] of every layer
    int o_p0;      // [NL][2D] the tap-0 chunks of conv_filter|conv_gate added in order, fg order
    int total;
};
__host__ __device__ inline WideLds wide_lds(const Layout& L, int R, int D)
{
    WideLds o;
    o.o_meta = 0;
    o.o_ctl = 192;
    o.o_hist = o.o_ctl + 16;
    o.o_x = o.o_hist + 64;
    o.o_z = o.o_x + 128;
    o.o_h1 = o.o_z + 128;
    o.o_h2 = o.o_h1 + L.S;
    o.o_lg = o.o_h2 + L.S;
    o.o_xold = o.o_lg + L.Opad;
    o.o_p0 = o.o_xold + L.NL * R;
    o.total = o.o_p0 + L.NL * 2 * D;
    return o;
}

// the last chunk of a contraction on the sample-to-sample path (AC-1b): chain 0 starts from the addend, chains 1-3 from their first
// product (an fma from -0); operand vector in LDS at float offset `xo`
__device__ __forceinline__ float dot_ldso_init(const Tile& t, int xo, float init)
{
    f32x2p s01 = {init, -0.0f}, s23 = {-0.0f, -0.0f};
#pragma unroll
    for (int kq = 0; kq < 8; ++kq) {
        const f32x4 q = LDS4((xo >> 2) + kq);
        s01 = pk_fma(f32x2p{t.w[4 * kq + 0], t.w[4 * kq + 1]}, f32x2p{q.x, q.y}, s01);
        s23 = pk_fma(f32x2p{t.w[4 * kq + 2], t.w[4 * kq + 3]}, f32x2p{q.z, q.w}, s23);
    }
    return (s01[0] + s01[1]) + (s23[0] + s23[1]);
}
// plain AC-1 over n chunks: tiles at base + c * kTile, operand at xo + 32 c; the next tile's loads are in flight under the current
// tile's fmas
__device__ __forceinline__ float cdot_tiles(const float* base, int n, int xo, int lane)
{
    Tile ta, tb;
    load_tile(ta, base, lane);
    float r = 0.0f;
    for (int c = 0; c < n; c += 2) {
        if (c + 1 < n) load_tile(tb, base + (long long)(c + 1) * kTile, lane);
        const float a0 = dot_ldso(ta, xo + c * 32);
        r = (c == 0) ? a0 : r + a0;
        if (c + 1 < n) {
            if (c + 2 < n) load_tile(ta, base + (long long)(c + 2) * kTile, lane);
            const float a1 = dot_ldso(tb, xo + (c + 1) * 32);
            r = r + a1;
        }
    }
    return r;
}
__device__ __forceinline__ unsigned wide_ring_pos(unsigned pos0, unsigned t, unsigned d)
{
    const unsigned v = pos0 + t;
    return (d & (d - 1)) == 0 ? (v & (d - 1)) : v % d;
}

}  // namespace

// =====================================================================================================
//  pack helpers
// =====================================================================================================
// vectors: dst[dst_off + g * dst_gs + i], i < n.  fg != 0: fg order, i = jb * 64 + lane -> lane < 32 ? A[32 jb + lane] : B[32 jb + lane - 32];
// else A[i] for i < ncols, 0 beyond
__global__ void wn_wide_pack_vec_kernel(float* dst, const float* src, long long dst_off, long long dst_gs, long long baseA, long long baseB,
                                        long long src_gs, int ngroups, int n, int ncols, int fg)
{
    const long long total = (long long)ngroups * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i / n), j = (int)(i % n);
        float v = 0.0f;
        if (fg) v = src[((j & 63) < 32 ? baseA : baseB) + (long long)g * src_gs + (j >> 6) * 32 + (j & 31)];
        else if (j < ncols) v = src[baseA + (long long)g * src_gs + j];
        dst[dst_off + (long long)g * dst_gs + j] = v;
    }
}

// =====================================================================================================
//  hoisted conditioning projections, 2D outputs per layer        (model.py:71-83, 181-212)
//  out[(row * NL + l) * 2D + jb * 64 + lane] = AC-1 over K terms of tiles [l][jb][c] with row `row` of the input
//  grid (ceil(rows / 8), NL), NFG waves; the 8 rows are staged (zero-padded to NC * 32) in LDS
// =====================================================================================================
constexpr int kWideProjRows = 8;
__global__ void __launch_bounds__(256) wn_wide_proj_kernel(const float* P, long long woff, long long wstride, int NC, int K, int NFG, int NL,
                                                           const float* in, const int32_t* ids, long long emb_off, long long rows, float* out)
{
    const int KP = NC * 32;
    const long long row0 = (long long)blockIdx.x * kWideProjRows;
    const int l = blockIdx.y;
    for (int i = threadIdx.x; i < kWideProjRows * KP; i += blockDim.x) {
        const int r = i / KP, k = i - r * KP;
        float v = 0.0f;
        if (row0 + r < rows && k < K) v = ids ? P[emb_off + (long long)ids[row0 + r] * K + k] : in[(row0 + r) * K + k];
        lds[i] = v;
    }
    __syncthreads();
    const int jb = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float acc[kWideProjRows];
    for (int c = 0; c < NC; ++c) {
        Tile t;
        load_tile(t, P + woff + (long long)l * wstride + (long long)(jb * NC + c) * kTile, lane);
#pragma unroll
        for (int r = 0; r < kWideProjRows; ++r) {
            const float a = dot_ldso(t, r * KP + c * 32);
            acc[r] = (c == 0) ? a : acc[r] + a;
        }
    }
#pragma unroll
    for (int r = 0; r < kWideProjRows; ++r)
        if (row0 + r < rows) out[((row0 + r) * NL + l) * ((long long)NFG * 64) + jb * 64 + lane] = acc[r];
}

// =====================================================================================================
//  the persistent generation kernel: one workgroup per stream
// =====================================================================================================
template <int RC, int DC, bool SCALAR, bool INSTR>
__global__ void __launch_bounds__(kWideThreads) wn_wide_generate_kernel(WideLaunch a)
{
    constexpr int R = RC * 32, D = DC * 32, D2 = 2 * D;
    constexpr int NFG = DC;                 // filter|gate output blocks
    constexpr int NDB = (R + 63) / 64;      // dense / causal output blocks
    constexpr int NSW = kWideWaves - NDB;   // skip waves
    const Layout& L = a.lay;
    const WideLayout& W = a.wl;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int NL = L.NL, S = L.S, NSJ = L.NSJ, NCH = L.NCH, T = a.T;
    const bool has_gc = L.G > 0, has_lc = L.L > 0, use_bias = L.use_bias != 0;
    const WideLds o = wide_lds(L, R, D);
    float* stb = a.state + (long long)b * L.state_stride;
    int* meta = reinterpret_cast<int*>(stb + L.st_meta);
    float* ring = stb + L.st_ring;
    const float* GCv = a.cond + (long long)b * NL * D2;
    const float* LCb = a.cond + (long long)a.B * NL * D2 + (long long)b * T * NL * D2;
    const int* pmeta = reinterpret_cast<const int*>(a.P + L.off_meta);
    const long long dbg_row = (long long)NL * (D + R) + L.Opad;
    const ActCoef coef = act_coef(lane >= 32);

    if (tid < 128) LDSI(o.o_meta + tid) = pmeta[tid];
    if (tid < 64) {
        LDSI(o.o_meta + 128 + tid) = reinterpret_cast<int*>(stb + L.st_ringpos)[tid];
        lds[o.o_hist + tid] = SCALAR ? stb[L.st_hist + tid] : 0.0f;
    }
    if (tid < 16) LDSI(o.o_ctl + tid) = 0;
    int prev_valid = meta[M_PREV_VALID], qprev = meta[M_QPREV];
    __syncthreads();

    float tot[2] = {0.0f, 0.0f};            // skip waves: running sum of the skip outputs of blocks (w - NDB) + k * NSW   (model.py:154)
    bool bad_any = false;

    for (int t = 0; t < T; ++t) {
        // ---------------- what does not need this step's layer outputs: x_l[t - d_l] of every layer, the input queue ----------------
        for (int i = tid; i < NL * R; i += kWideThreads) {
            const int l = i / R, r = i - l * R;
            const unsigned d = (unsigned)LDSI(o.o_meta + l);
            const unsigned pos = wide_ring_pos((unsigned)LDSI(o.o_meta + 128 + l), (unsigned)t, d);
            lds[o.o_xold + i] = ring[LDSI(o.o_meta + 64 + l) + (long long)pos * R + r];
        }
        int qcur = 0;
        if (SCALAR) {
            if (w == kWideWaves - 1) {
                // model.py:122 causal_queue shift + append
                float s_in;
                if (a.forced != nullptr) s_in = reinterpret_cast<const float*>(a.forced)[(long long)b * T + t];
                else if (t == 0) s_in = reinterpret_cast<const float*>(a.first_input)[b];
                else s_in = lds[o.o_ctl];
                const float v = (lane + 1 < L.ifw) ? lds[o.o_hist + lane + 1] : s_in;
                if (lane < L.ifw) lds[o.o_hist + lane] = v;
            }
        } else {
            if (a.forced != nullptr) qcur = reinterpret_cast<const int*>(a.forced)[(long long)b * T + t];
            else if (t == 0) qcur = reinterpret_cast<const int*>(a.first_input)[b];
            else qcur = LDSI(o.o_ctl);
        }
        __syncthreads();
        // ---------------- tap-0 chunks of conv_filter|conv_gate of ALL layers (x[t-d] is at least one step old), causal layer ----------------
        for (int k = w; k < NL * NFG; k += kWideWaves) {
            const int l = k / NFG, jb = k - l * NFG;
            const float* fg = a.P + W.off_layer0 + (long long)l * W.layer_stride + W.l_fg + (long long)jb * (2 * RC) * kTile;
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                Tile tl;
                load_tile(tl, fg + c * kTile, lane);
                const float v = dot_ldso(tl, o.o_xold + l * R + c * 32);
                acc = (c == 0) ? v : acc + v;
            }
            lds[o.o_p0 + l * D2 + jb * 64 + lane] = acc;
        }
        if (SCALAR) {
            // model.py:131 / 41-46 causal layer: AC-1 over the ifw queue entries, no bias
            if (w < NDB) {
                const float x0 = cdot_tiles(a.P + W.off_causal + (long long)w * L.NCA * kTile, L.NCA, o.o_hist, lane);
                if (w * 64 + lane < R) lds[o.o_x + w * 64 + lane] = x0;
            }
        } else {
            // one-hot input: the k=2 causal conv over one-hot rows is the sum of two kernel rows
            if (tid < R) {
                const float w1r = a.P[W.off_causal + ((long long)L.Q + qcur) * R + tid];
                float x0 = w1r;
                if (prev_valid) x0 = a.P[W.off_causal + (long long)qprev * R + tid] + w1r;
                lds[o.o_x + tid] = x0;
            }
            qprev = qcur; prev_valid = 1;
        }
        __syncthreads();

        // ---------------- the dilated residual stack (model.py:112-149) ----------------
        // lc frame used at step t = frame pushed at step t-1 (model.py:79-80: slice from the FRONT of the queue)
        const float* lcrow = (t == 0) ? (stb + L.st_lcprev) : (LCb + (long long)(t - 1) * NL * D2);
        for (int l = 0; l < NL; ++l) {
            const float* lw = a.P + W.off_layer0 + (long long)l * W.layer_stride;
            if (w < NFG) {
                // model.py:68-69 conv_filter|conv_gate: head = tap-0 chunks, then the tap-1 chunks but the last, in order;
                // addend ((head + bias) + gc) + lc; the last chunk starts from the addend (AC-1b)
                const int jb = w;
                const float* fg = lw + W.l_fg + (long long)jb * (2 * RC) * kTile;
                const float bv = use_bias ? lw[W.l_bfg + jb * 64 + lane] : 0.0f;
                const float gv = has_gc ? GCv[l * D2 + jb * 64 + lane] : 0.0f;
                const float lv = has_lc ? lcrow[l * D2 + jb * 64 + lane] : 0.0f;
                float acc = lds[o.o_p0 + l * D2 + jb * 64 + lane];
#pragma unroll
                for (int c = 0; c < RC - 1; ++c) {
                    Tile tl;
                    load_tile(tl, fg + (RC + c) * kTile, lane);
                    acc = acc + dot_ldso(tl, o.o_x + c * 32);
                }
                if (use_bias) acc = acc + bv;
                if (has_gc) acc = acc + gv;      // model.py:71-73
                if (has_lc) acc = acc + lv;      // model.py:75-83
                Tile tl;
                load_tile(tl, fg + (2 * RC - 1) * kTile, lane);
                const float v = dot_ldso_init(tl, o.o_x + (RC - 1) * 32, acc);
                // model.py:86 tanh(filter) * sigmoid(gate): lanes 0-31 hold tanh, lanes 32-63 the logistic of the same channels
                const float act = act_eval(coef, v);
                const float oth = __shfl(act, lane ^ 32);
                const float z = act * oth;
                if (lane < 32) {
                    lds[o.o_z + jb * 32 + lane] = z;
                    if (INSTR && a.dbg != nullptr && t < a.dbg_steps)
                        a.dbg[((long long)b * a.dbg_steps + t) * dbg_row + (long long)l * (D + R) + jb * 32 + lane] = z;
                }
            } else if (tid - NFG * 64 < R) {
                // model.py:145 dilation queue <- the layer INPUT x[t] (the row read as x[t-d] in this step's first phase)
                const int r = tid - NFG * 64;
                const unsigned d = (unsigned)LDSI(o.o_meta + l);
                const unsigned pos = wide_ring_pos((unsigned)LDSI(o.o_meta + 128 + l), (unsigned)t, d);
                ring[LDSI(o.o_meta + 64 + l) + (long long)pos * R + r] = lds[o.o_x + r];
            }
            __syncthreads();
            if (w < NDB) {
                // model.py:89 dense 1x1: head chunks in order (0.0f when there is none), + bias, last chunk from that addend (AC-1b)
                const float* wd = lw + W.l_wd + (long long)w * DC * kTile;
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < DC - 1; ++c) {
                    Tile tl;
                    load_tile(tl, wd + c * kTile, lane);
                    const float v = dot_ldso(tl, o.o_z + c * 32);
                    acc = (c == 0) ? v : acc + v;
                }
                if (use_bias) acc = acc + lw[W.l_bd + w * 64 + lane];
                Tile tl;
                load_tile(tl, wd + (DC - 1) * kTile, lane);
                const float tr = dot_ldso_init(tl, o.o_z + (DC - 1) * 32, acc);
                const int r = w * 64 + lane;
                if (r < R) {
                    const float xn = lds[o.o_x + r] + tr;      // model.py:98-101 residual
                    lds[o.o_x + r] = xn;
                    if (INSTR && a.dbg != nullptr && t < a.dbg_steps)
                        a.dbg[((long long)b * a.dbg_steps + t) * dbg_row + (long long)l * (D + R) + D + r] = xn;
                }
            } else if (a.forced == nullptr) {
                // model.py:96 skip 1x1: plain AC-1 over D/32 chunks, + bias; model.py:154 running sum in layer order
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int jb = (w - NDB) + k * NSW;
                    if (jb < NSJ) {
                        const float* sk = lw + W.l_sk + (long long)jb * DC * kTile;
                        float acc = 0.0f;
#pragma unroll
                        for (int c = 0; c < DC; ++c) {
                            Tile tl;
                            load_tile(tl, sk + c * kTile, lane);
                            const float v = dot_ldso(tl, o.o_z + c * 32);
                            acc = (c == 0) ? v : acc + v;
                        }
                        if (use_bias) acc = acc + lw[W.l_bs + jb * 64 + lane];
                        tot[k] = (l == 0) ? acc : tot[k] + acc;
                    }
                }
            }
            __syncthreads();
        }
        if (a.forced != nullptr) continue;      // priming (generate.py:177-180): the queues are all that matters

        // ---------------- model.py:150-165 postprocessing ----------------
        if (w >= NDB) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int jb = (w - NDB) + k * NSW;
                if (jb < NSJ) lds[o.o_h1 + jb * 64 + lane] = tot[k] > 0.0f ? tot[k] : 0.0f;      // model.py:157
            }
        }
        __syncthreads();
        for (int jb = w; jb < NSJ; jb += kWideWaves) {
            float v = cdot_tiles(a.P + L.off_w1 + (long long)jb * NCH * kTile, NCH, o.o_h1, lane);     // model.py:158
            if (use_bias) v = v + a.P[L.off_b1 + jb * 64 + lane];
            lds[o.o_h2 + jb * 64 + lane] = v > 0.0f ? v : 0.0f;                                        // model.py:160
        }
        __syncthreads();
        for (int ob = w; ob < L.NOJ; ob += kWideWaves) {
            float y = cdot_tiles(a.P + L.off_w2 + (long long)ob * NCH * kTile, NCH, o.o_h2, lane);     // model.py:161-165
            if (use_bias && ob * 64 + lane < L.O) y = y + a.P[L.off_b2 + ob * 64 + lane];
            lds[o.o_lg + ob * 64 + lane] = y;
            if (INSTR && a.dbg != nullptr && t < a.dbg_steps)
                a.dbg[((long long)b * a.dbg_steps + t) * dbg_row + (long long)NL * (D + R) + ob * 64 + lane] = y;
        }
        __syncthreads();
        if (w == 0) {
            if (SCALAR) {
                // mixture.py:84-114 sample_from_discretized_mix_logistic, uniforms injected: the CPU checker's statements in order
                const int nr = L.nr_mix;
                const float* up = reinterpret_cast<const float*>(a.uniforms) + ((long long)b * T + t) * (nr + 1);
                const float u = lane <= nr ? up[lane] : 0.5f;
                const float y = lds[o.o_lg + lane];
                const float gmb = y - log_e(-log_e(u));                        // mixture.py:103 (lanes < nr)
                int k = 0;
                float best = __shfl(gmb, 0);
                for (int i = 1; i < nr; ++i) {
                    const float gi = __shfl(gmb, i);
                    if (gi > best) { best = gi; k = i; }                       // first maximum
                }
                const float mean = __shfl(y, nr + k);                          // mixture.py:105
                float ls = __shfl(y, 2 * nr + k);                              // mixture.py:107
                const float lsmin = (float)-32.23619130191664;
                ls = ls > lsmin ? ls : lsmin;
                const float uu = __shfl(u, nr);
                const float tq = log_e(uu) - log_e(1.0f - uu);                 // mixture.py:111
                const float e = exp_e(ls);
                const float prod = e * tq;
                float xs = mean + prod;
                xs = xs > -1.0f ? xs : -1.0f;                                  // mixture.py:113
                xs = xs < 1.0f ? xs : 1.0f;
                if (lane == 0) {
                    reinterpret_cast<float*>(a.out)[(long long)b * T + t] = xs;
                    lds[o.o_ctl] = xs;
                }
            } else {
                // model.py:243 float64 softmax -> float32, generate.py:219-222 temperature, generate.py:231 np.random.choice (AC-5)
                const int Q = L.Q;
                float xv[16];                                                  // lane owns classes lane + 64 k
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = lane + 64 * k;
                    xv[k] = (i < Q) ? lds[o.o_lg + i] : 0.0f;
                }
                const double uu = reinterpret_cast<const double*>(a.uniforms)[(long long)b * T + t];
                bool bad = false;
                const int idx = categorical_sample<16>(xv, Q, lane, a.temperature, uu, nullptr, nullptr, &bad);
                bad_any = bad_any || bad;
                if (lane == 0) {
                    reinterpret_cast<int*>(a.out)[(long long)b * T + t] = idx;
                    LDSI(o.o_ctl) = idx;
                }
            }
        }
        __syncthreads();
    }

    // ---------------- persist the per-stream state (model.py:49-64 queues) ----------------
    __syncthreads();
    if (tid < 64) {
        const unsigned d = (unsigned)LDSI(o.o_meta + tid);
        reinterpret_cast<int*>(stb + L.st_ringpos)[tid] = (int)(((unsigned)LDSI(o.o_meta + 128 + tid) + (unsigned)T) % (d ? d : 1u));
        if (SCALAR) stb[L.st_hist + tid] = lds[o.o_hist + tid];
    }
    if (tid == 0) {
        meta[M_TABS] = meta[M_TABS] + T;
        meta[M_PREV_VALID] = prev_valid;
        meta[M_QPREV] = qprev;
        if (bad_any) atomicMax(a.status, 31);      // NaN probabilities: np.random.choice would raise (generate.py:231)
    }
    if (has_lc && T > 0) {
        const float* last = LCb + (long long)(T - 1) * NL * D2;
        for (int i = tid; i < NL * D2; i += kWideThreads) stb[L.st_lcprev + i] = last[i];
    }
}

// =====================================================================================================
//  host side
// =====================================================================================================
namespace twv {

long long wide_build_packed_layout(Layout& L, WideLayout& wl, int R, int D)
{
    wl.R = R; wl.D = D; wl.RC = R / 32; wl.DC = D / 32; wl.NFG = D / 32; wl.NDB = (R + 63) / 64;
    long long p = 0;
    L.off_meta = p; p += 128;
    wl.off_causal = p; p += L.scalar ? (long long)wl.NDB * L.NCA * kTile : (long long)2 * L.Q * R;
    L.off_causal = wl.off_causal;
    long long q = 0;
    wl.l_fg = q; q += (long long)wl.NFG * 2 * wl.RC * kTile;
    wl.l_wd = q; q += (long long)wl.NDB * wl.DC * kTile;
    wl.l_sk = q; q += (long long)L.NSJ * wl.DC * kTile;
    wl.l_bfg = q; q += wl.NFG * 64;
    wl.l_bd = q; q += wl.NDB * 64;
    wl.l_bs = q; q += L.S;
    wl.off_layer0 = p; wl.layer_stride = q;
    L.off_layer0 = p; L.layer_stride = q;
    p += q * L.NL;
    L.off_w1 = p; p += (long long)L.NSJ * L.NCH * kTile;
    L.off_b1 = p; p += L.S;
    L.off_w2 = p; p += (long long)L.NOJ * L.NCH * kTile;
    L.off_b2 = p; p += L.Opad;
    L.off_lcw = p; L.lcw_stride = (long long)wl.NFG * L.NLC * kTile; p += L.lcw_stride * L.NL;
    L.off_gcw = p; L.gcw_stride = (long long)wl.NFG * L.NGC * kTile; p += L.gcw_stride * L.NL;
    L.off_gcemb = p; p += ((long long)L.gc_card * L.G + 3) / 4 * 4;
    for (int i = 0; i < L.n_up; ++i) { L.off_up[i] = p; p += ((long long)L.up[i] * 2 + 3) / 4 * 4; }
    L.off_xl = 0; L.off_xc = 0;
    L.packed_floats = p;
    return p;
}

static inline int wide_grid(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// the meta words (dilations, delay-line offsets) are written by the caller
int wide_pack(float* dst, const float* blob, const Layout& L, const WideLayout& wl, hipStream_t st)
{
    const int R = wl.R, D = wl.D;
    const long long ls = wl.layer_stride, cs = L.c_layer_stride, c0 = L.c_layer0, l0 = wl.off_layer0;
    auto tiles = [&](long long dst_off, long long dst_gs, long long baseA, long long baseB, long long src_gs, int ng, int njb, int nch,
                     int K, int rowlen, int ncols, int halves) {
        PackTiles p{dst_off, dst_gs, baseA, baseB, src_gs, ng, njb, nch, K, rowlen, ncols, halves, 64};
        twv_launch_pack_tiles(dst, blob, p, st);
    };
    auto vec = [&](long long dst_off, long long dst_gs, long long baseA, long long baseB, long long src_gs, int ng, int n, int ncols, int fg) {
        hipLaunchKernelGGL(wn_wide_pack_vec_kernel, dim3(wide_grid((long long)ng * n)), dim3(256), 0, st, dst, blob, dst_off, dst_gs, baseA, baseB,
                           src_gs, ng, n, ncols, fg);
    };
    if (L.scalar) tiles(wl.off_causal, 0, L.c_causal, 0, 0, 1, wl.NDB, L.NCA, L.ifw, R, R, 0);      // wavenet/conv1d/kernel (ifw,1,R)
    else twv_launch_copy(dst + wl.off_causal, blob + L.c_causal, (long long)2 * L.Q * R, st);          // (2,Q,R)
    for (int jb = 0; jb < wl.NFG; ++jb) {
        // conv_filter|conv_gate kernels (2,R,D): rows tap * R + r; block jb = channels [32 jb, 32 jb + 32) of both
        tiles(l0 + wl.l_fg + (long long)jb * 2 * wl.RC * kTile, ls, c0 + L.c_wf + jb * 32, c0 + L.c_wg + jb * 32, cs, L.NL, 1, 2 * wl.RC,
              2 * R, D, D, 1);
        if (L.L) tiles(L.off_lcw + (long long)jb * L.NLC * kTile, L.lcw_stride, c0 + L.c_lcf + jb * 32, c0 + L.c_lcg + jb * 32, cs, L.NL, 1,
                       L.NLC, L.L, D, D, 1);
        if (L.G) tiles(L.off_gcw + (long long)jb * L.NGC * kTile, L.gcw_stride, c0 + L.c_gcf + jb * 32, c0 + L.c_gcg + jb * 32, cs, L.NL, 1,
                       L.NGC, L.G, D, D, 1);
    }
    tiles(l0 + wl.l_wd, ls, c0 + L.c_wd, 0, cs, L.NL, wl.NDB, wl.DC, D, R, R, 0);                     // dense kernel (1,D,R)
    tiles(l0 + wl.l_sk, ls, c0 + L.c_ws, 0, cs, L.NL, L.NSJ, wl.DC, D, L.S, L.S, 0);                  // skip kernel (1,D,S)
    if (L.use_bias) {
        vec(l0 + wl.l_bfg, ls, c0 + L.c_bf, c0 + L.c_bg, cs, L.NL, wl.NFG * 64, 0, 1);
        vec(l0 + wl.l_bd, ls, c0 + L.c_bd, 0, cs, L.NL, wl.NDB * 64, R, 0);
        vec(l0 + wl.l_bs, ls, c0 + L.c_bs, 0, cs, L.NL, L.S, L.S, 0);
        vec(L.off_b1, 0, L.c_b1, 0, 0, 1, L.S, L.S, 0);
        vec(L.off_b2, 0, L.c_b2, 0, 0, 1, L.Opad, L.O, 0);
    }
    tiles(L.off_w1, 0, L.c_w1, 0, 0, 1, L.NSJ, L.NCH, L.S, L.S, L.S, 0);                              // conv1d_1 kernel (1,S,S)
    tiles(L.off_w2, 0, L.c_w2, 0, 0, 1, L.NOJ, L.NCH, L.S, L.O, L.O, 0);                              // conv1d_2 kernel (1,S,O)
    if (L.G) twv_launch_copy(dst + L.off_gcemb, blob + L.c_gcemb, (long long)L.gc_card * L.G, st);
    for (int i = 0; i < L.n_up; ++i) twv_launch_copy(dst + L.off_up[i], blob + L.c_up[i], (long long)L.up[i] * 2, st);
    if (hipGetLastError() != hipSuccess) return twv_fail(TWV_E_HIP, "wide pack launch failed");
    return TWV_OK;
}

int wide_condition(const float* P, const Layout& L, const WideLayout& wl, const float* upsampled, const int32_t* gc_ids, int batch,
                   int n_steps, float* cond, hipStream_t st)
{
    const int D2 = 2 * wl.D;
    float* GCv = cond;
    float* LC = GCv + (size_t)batch * L.NL * D2;
    if (L.G) {
        if (!gc_ids) return twv_fail(TWV_E_INVALID, "gc_ids required (generate.py:72-77)");
        // model.py:191-207: ids looked up in gc_embedding, or (no cardinality) the embedding itself as (B, G) floats through the same pointer
        const bool lookup = L.gc_card > 0;
        dim3 grid((unsigned)((batch + kWideProjRows - 1) / kWideProjRows), (unsigned)L.NL);
        hipLaunchKernelGGL(wn_wide_proj_kernel, grid, dim3(wl.NFG * 64), (size_t)kWideProjRows * L.NGC * 32 * 4, st, P, L.off_gcw, L.gcw_stride,
                           L.NGC, L.G, wl.NFG, L.NL, lookup ? (const float*)nullptr : reinterpret_cast<const float*>(gc_ids),
                           lookup ? gc_ids : (const int32_t*)nullptr, L.off_gcemb, (long long)batch, GCv);
    } else {
        if (hipMemsetAsync(GCv, 0, (size_t)batch * L.NL * D2 * 4, st) != hipSuccess) return twv_fail(TWV_E_HIP, "hipMemsetAsync failed");
    }
    if (L.L && n_steps > 0) {
        if (!upsampled) return twv_fail(TWV_E_INVALID, "upsampled local condition required");
        const long long rows = (long long)batch * n_steps;
        dim3 grid((unsigned)((rows + kWideProjRows - 1) / kWideProjRows), (unsigned)L.NL);
        hipLaunchKernelGGL(wn_wide_proj_kernel, grid, dim3(wl.NFG * 64), (size_t)kWideProjRows * L.NLC * 32 * 4, st, P, L.off_lcw, L.lcw_stride,
                           L.NLC, L.L, wl.NFG, L.NL, upsampled, (const int32_t*)nullptr, 0LL, rows, LC);
    }
    if (hipGetLastError() != hipSuccess) return twv_fail(TWV_E_HIP, "wide conditioning launch failed");
    return TWV_OK;
}

template <int RC, int DC, bool SCALAR, bool INSTR>
static int wide_launch3(const WideLaunch& a, size_t shm, hipStream_t st)
{
    auto kern = wn_wide_generate_kernel<RC, DC, SCALAR, INSTR>;
    if (shm > 32 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
        return twv_fail(TWV_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(kWideThreads), shm, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return twv_fail(TWV_E_HIP, std::string("wn_wide_generate_kernel launch: ") + hipGetErrorString(e));
    return TWV_OK;
}
// the instrumented build (per-layer dumps) is a separate instantiation: production launches carry none of its branches
template <int RC, int DC>
static int wide_launch2(const WideLaunch& a, size_t shm, hipStream_t st)
{
    if (a.lay.scalar) return a.dbg ? wide_launch3<RC, DC, true, true>(a, shm, st) : wide_launch3<RC, DC, true, false>(a, shm, st);
    return a.dbg ? wide_launch3<RC, DC, false, true>(a, shm, st) : wide_launch3<RC, DC, false, false>(a, shm, st);
}

int wide_launch(const WideLaunch& a, hipStream_t st)
{
    const WideLds o = wide_lds(a.lay, a.wl.R, a.wl.D);
    const size_t shm = (size_t)o.total * 4;
    if (shm > (size_t)kWideLdsBytes) return twv_fail(TWV_E_UNSUPPORTED, "model does not fit the 160 KiB LDS budget of the wide kernel");
    switch (a.wl.RC * 8 + a.wl.DC) {
    case 1 * 8 + 2: return wide_launch2<1, 2>(a, shm, st);
    case 1 * 8 + 4: return wide_launch2<1, 4>(a, shm, st);
    case 2 * 8 + 1: return wide_launch2<2, 1>(a, shm, st);
    case 2 * 8 + 2: return wide_launch2<2, 2>(a, shm, st);
    case 2 * 8 + 4: return wide_launch2<2, 4>(a, shm, st);
    case 4 * 8 + 1: return wide_launch2<4, 1>(a, shm, st);
    case 4 * 8 + 2: return wide_launch2<4, 2>(a, shm, st);
    case 4 * 8 + 4: return wide_launch2<4, 4>(a, shm, st);
    }
    return twv_fail(TWV_E_UNSUPPORTED, "residual_channels and dilation_channels must each be 32, 64 or 128");
}

bool wide_fits_lds(const Layout& L, int R, int D) { return (size_t)wide_lds(L, R, D).total * 4 <= (size_t)kWideLdsBytes; }

}  // namespace twv
