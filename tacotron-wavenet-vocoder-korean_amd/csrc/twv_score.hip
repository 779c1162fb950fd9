// twv_score.hip -- MI355X (gfx950) WaveNet scoring: per-sample negative log-likelihood of given audio + its C-ABI (include/twv_amd.h).
//
// Scoring is the reference's add_loss graph with reduce=False (citations into hccho2/Tacotron-Wavenet-Vocoder-Korean):
//   wavenet/model.py:247-312  add_loss: drop the last sample, create_upsample, the 'valid' convolution network (model.py:112-167,
//                             train_mode=True, local condition sliced from the FRONT of every layer, model.py:79-80), targets audio[rf:]
//   wavenet/mixture.py:27-81  discretized_mix_logistic_loss(num_class=2**16, reduce=False);  model.py:257-296 the one-hot model's
//                             softmax cross-entropy
// -- NOT the incremental (generation) graph.  A call scores one batch of WINDOWS: slot b holds len_b <= window samples (a hop
// multiple > rf, or 0 = idle) and gets nll[b][p], p < len_b - rf, the loss terms of the training graph on that crop.  Whole utterances
// are cut into hop-aligned windows with a receptive-field halo by the host (score.py); DESIGN.md 3s' has the argument why that is exact.
//
// Layout: a slot's rows start at its first sample (row t of layer l exists for off[l] <= t < len_b - 1), so a shorter slot is the same
// picture with fewer rows: the skip slice starts at row rf - 1 whatever the length.  The residual stack is ONE forward-only kernel per
// layer (sc_layer_fwd_kernel: the MFMA scheme of the training step's tr_layer_fwd_kernel, no TH / SG, X ping-pongs between two
// buffers, rows outside a slot load nothing and store nothing); its skip inputs go to the stacked ZC columns that the head consumes.
// Front (weight views, unfold / one-hot gather, gc gather, upsampler stages or ctab / Q) and head (stacked skip GEMM, conv1d_1,
// conv1d_2) are the training step's own: wavenet_forward_front / wavenet_forward_head (twv_wavenet_graph.hpp, defined in twv_train.hip
// beside their kernels).  The same header holds the model description both handles embed: geometry, canonical offsets, refusals, route.
// The loss kernels write per-row terms only: no gradient, no mean.
// residual_channels = dilation_channels = 64 and 128 take the same front, head and loss kernels and sc_layer_wide_fwd_kernel<W, FUSED>
// per layer; width 32 runs sc_layer_fwd_kernel as before.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_dev.hpp"
#include "twv_wavenet_graph.hpp"

struct twv_wavenet_scorer {
    WavenetGraph g;                                          // rows = slots, T = window samples
    rocblas_handle blas;
    long long carve_floats;
    std::string route;
};

// ---------------------------------------------------------------------------------------------------------------
//  kernels
// ---------------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4t __attribute__((ext_vector_type(4)));
typedef float f32x2t __attribute__((ext_vector_type(2)));
#define GRID_STRIDE(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

// the training step's activations (v_exp_f32 / v_rcp_f32, ~1e-6 relative): scoring is held to the same float32 bar
__device__ __forceinline__ float sc_sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float sc_tanh_fast(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }
__device__ __forceinline__ f32x4t sc_ld4(const float* p, bool ok) { f32x4t z = {0.f, 0.f, 0.f, 0.f}; return ok ? *reinterpret_cast<const f32x4t*>(p) : z; }

// ===================================================================================================================
//  Forward-only gated layer (model.py:66-101 train mode) on the f32 matrix cores, the scheme of tr_layer_fwd_kernel:
//  one wave owns 32-row tiles (rows = consecutive t of one slot); per tile
//      pre[32 x 64] = X[t-d] W0 + X[t] W1 + lc term          v_mfma_f32_32x32x2_f32, B operands (filter, gate) from LDS
//      z = tanh(pre_f + bias + gc) * sigmoid(pre_g + bias + gc);   x_next = X[t] + z Wd + bd   (z: C layout -> A layout through LDS)
//  FUSED: lc term = sum_j ctab[phase(t - o)][j] * Q_j[frame(t - o)] (frame-rate projections, hop >= 32: at most two frames per tile);
//  else 80 more k-steps over the materialised upsampler rows U[t - o].
//  A row is touched only if it exists: o <= t < len_b - 1 (o = the layer's output offset).  Every load of a row that does not exist is
//  predicated off (the operand is 0) and nothing is stored for it, so the workspace needs no clearing and a shorter or idle slot
//  cannot reach its neighbour's rows.  Writes x_next and, for rows t >= rf - 1, the layer's 32 columns of the stacked skip input ZC.
// ===================================================================================================================
struct ScLayerArgs {
    const float* X; const float* U; const float* gcp;        // (slots*Tn,32) (slots*T,80) (slots,64)
    const float* W0; const float* W1; const float* Wlc;      // views (32,64) (32,64) (80,64): columns filter | gate
    const float* Wd;                                         // (32,32)
    const float* bf; const float* bg; const float* bd;       // nullable
    float* XN; float* ZC;                                    // ZC already offset to this layer's 32 columns
    const int32_t* lens;                                     // (slots) samples per slot, 0 = idle
    int slots, T, Tn, d, o, cut, ow, ldz, tpb, t_lo;         // cut = rf - 1; tiles walked per slot start at row t_lo = (o / 32) * 32
    const float* Q; const float* ctab; int hop, F;           // FUSED: Q[((b*F + frame)*4 + j)*64 + column], ctab[phase*4 + j]
};
constexpr int kScLcSteps = 10;                               // 80 / 8
constexpr int kScSteps = 32 + 4 * kScLcSteps;                // tap0 16 + tap1 16 + lc 40 MFMA steps per column half

template <bool FUSED>
__global__ void __launch_bounds__(512) sc_layer_fwd_kernel(ScLayerArgs a)
{
    __shared__ float bt[(FUSED ? 32 : kScSteps) * 128];      // [step][lane][filter, gate]
    __shared__ __attribute__((aligned(16))) float cts[FUSED ? 4 * 512 : 4];   // ctab (hop <= 512)
    __shared__ float bdt[16 * 64];                           // dense: [step][lane]
    __shared__ __attribute__((aligned(16))) float zt[8][32 * 36];
    if (FUSED) for (int e = threadIdx.x; e < a.hop * 4; e += 512) cts[e] = a.ctab[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 31, hh = lane >> 5;
    for (int e = threadIdx.x; e < (FUSED ? 32 : kScSteps) * 64; e += 512) {
        const int s = e >> 6, l = e & 63, nn = l & 31, h2 = l >> 5;
        const float* W; int ij;
        if (s < 16) { W = a.W0; ij = s; } else if (s < 32) { W = a.W1; ij = s - 16; } else { W = a.Wlc; ij = s - 32; }
        const int k = 8 * (ij >> 2) + 4 * h2 + (ij & 3);
        bt[e * 2] = W[k * 64 + nn]; bt[e * 2 + 1] = W[k * 64 + 32 + nn];
    }
    for (int e = threadIdx.x; e < 16 * 64; e += 512) {
        const int s = e >> 6, l = e & 63;
        bdt[e] = a.Wd[(8 * (s >> 2) + 4 * (l >> 5) + (s & 3)) * 32 + (l & 31)];
    }
    __syncthreads();
    const float vbf = a.bf ? a.bf[n] : 0.0f, vbg = a.bg ? a.bg[n] : 0.0f, vbd = a.bd ? a.bd[n] : 0.0f;
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int ntiles = a.slots * a.tpb, nwaves = gridDim.x * 8;
    for (int tile = blockIdx.x * 8 + wave; tile < ntiles; tile += nwaves) {
        const int b = tile / a.tpb, t0 = (tile - b * a.tpb) * 32 + a.t_lo;
        const int Tb = a.lens[b] - 1;                        // the slot's rows: its last sample is a target only (idle slot: -1)
        if (t0 >= Tb) continue;                              // wave-uniform: the whole tile lies behind the slot's end (zt is wave-private)
        // ---- A operands: lane (row, hh) carries k = 8i + 4hh .. +3 of its row
        f32x4t x0[4], x1[4], u[FUSED ? 1 : kScLcSteps];
        {
            const int t = t0 + n;
            const bool ok = t < Tb && t >= a.o;
            const float* xr = a.X + ((long long)b * a.Tn + t) * 32 + 4 * hh;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x0[i] = sc_ld4(xr - (long long)a.d * 32 + 8 * i, ok);      // t - d >= off[l]: a row of the layer's input
                x1[i] = sc_ld4(xr + 8 * i, ok);
            }
            if (!FUSED) {
                const float* ur = a.U + ((long long)b * a.T + (t - a.o)) * 80 + 4 * hh;
#pragma unroll
                for (int i = 0; i < kScLcSteps; ++i) u[i] = sc_ld4(ur + 8 * i, ok);
            }
        }
        // residual operand and gc projection in the output (C) layout: lane = channel n, register r = row (r&3) + 8(r>>2) + 4hh
        const float gcf = a.gcp ? a.gcp[b * 64 + n] : 0.0f, gcg = a.gcp ? a.gcp[b * 64 + 32 + n] : 0.0f;
        float xres[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            xres[r] = (t < Tb && t >= a.o) ? a.X[((long long)b * a.Tn + t) * 32 + n] : 0.0f;
        }
        f32x16 cf = zero, cg = zero;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2t w = *reinterpret_cast<const f32x2t*>(&bt[((4 * i + j) * 64 + lane) * 2]);
                cf = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[i][j], w[0], cf, 0, 0, 0);
                cg = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[i][j], w[1], cg, 0, 0, 0);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2t w = *reinterpret_cast<const f32x2t*>(&bt[((16 + 4 * i + j) * 64 + lane) * 2]);
                cf = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[i][j], w[0], cf, 0, 0, 0);
                cg = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[i][j], w[1], cg, 0, 0, 0);
            }
        if (!FUSED) {
#pragma unroll
            for (int i = 0; i < kScLcSteps; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x2t w = *reinterpret_cast<const f32x2t*>(&bt[((32 + 4 * i + j) * 64 + lane) * 2]);
                    cf = __builtin_amdgcn_mfma_f32_32x32x2f32(u[i][j], w[0], cf, 0, 0, 0);
                    cg = __builtin_amdgcn_mfma_f32_32x32x2f32(u[i][j], w[1], cg, 0, 0, 0);
                }
        } else {
            // rows of the tile: U row u = t - o; at most two frames per 32-row tile (hop >= 32).  fA < F: t0 < Tb <= T - 1.
            int u0 = t0 - a.o; u0 = u0 < 0 ? 0 : u0;
            const int fA = u0 / a.hop, fB = fA + 1 < a.F ? fA + 1 : fA;
            const int edge = (fA + 1) * a.hop;                               // first U row of frame fA + 1
            const float* qa = a.Q + (((long long)b * a.F + fA) * 4) * 64 + n;
            const float* qb = a.Q + (((long long)b * a.F + fB) * 4) * 64 + n;
            float qfa[4], qga[4], qfb[4], qgb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { qfa[j] = qa[j * 64]; qga[j] = qa[j * 64 + 32]; qfb[j] = qb[j * 64]; qgb[j] = qb[j * 64 + 32]; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int uu = t0 - a.o + (r & 3) + 8 * (r >> 2) + 4 * hh;
                uu = uu < 0 ? 0 : uu;                                         // rows below the layer's offset are discarded by the epilogue
                const bool hi = uu >= edge;
                int ph = uu - (hi ? edge : edge - a.hop);
                ph = ph < a.hop ? ph : a.hop - 1;                             // (only rows past the window's end, discarded as well)
                const f32x4t c = *reinterpret_cast<const f32x4t*>(&cts[ph * 4]);
                const float f0 = hi ? qfb[0] : qfa[0], f1 = hi ? qfb[1] : qfa[1], f2 = hi ? qfb[2] : qfa[2], f3 = hi ? qfb[3] : qfa[3];
                const float g0 = hi ? qgb[0] : qga[0], g1 = hi ? qgb[1] : qga[1], g2 = hi ? qgb[2] : qga[2], g3 = hi ? qgb[3] : qga[3];
                cf[r] += ((c[0] * f0 + c[1] * f1) + c[2] * f2) + c[3] * f3;
                cg[r] += ((c[0] * g0 + c[1] * g1) + c[2] * g2) + c[3] * g3;
            }
        }
        // ---- gated unit; rows that do not exist give z = 0 (a select, not a product: whatever their accumulators hold)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * hh, t = t0 + rl;
            const bool valid = t < Tb && t >= a.o;
            const float th = sc_tanh_fast((cf[r] + vbf) + gcf), sg = sc_sigmoid_fast((cg[r] + vbg) + gcg);
            const float z = valid ? th * sg : 0.0f;
            if (valid && t >= a.cut) a.ZC[((long long)b * a.ow + (t - a.cut)) * a.ldz + n] = z;       // model.py:94-96: the last len_b - rf rows
            zt[wave][rl * 36 + n] = z;
        }
        // ---- dense 1x1 + residual: z as A operand (row layout) back from this wave's LDS patch
        f32x16 cd = zero;
        {
            const float* zr = &zt[wave][n * 36 + 4 * hh];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4t q = *reinterpret_cast<const f32x4t*>(zr + 8 * i);
#pragma unroll
                for (int j = 0; j < 4; ++j) cd = __builtin_amdgcn_mfma_f32_32x32x2f32(q[j], bdt[(4 * i + j) * 64 + lane], cd, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (t < Tb && t >= a.o) a.XN[((long long)b * a.Tn + t) * 32 + n] = (xres[r] + cd[r]) + vbd;
        }
    }
}

// ===================================================================================================================
//  The same layer at residual = dilation width W = 64 or 128 (ScLayerArgs with W for every 32 and 2W for every 64: X, XN (slots*Tn, W);
//  views W0, W1 (W, 2W), Wlc (80, 2W), columns filter | gate; Wd (W, W); gcp (slots, 2W); Q[((b*F + frame)*4 + j)*2W + column]; ZC
//  already offset to the layer's W columns).  The contract is sc_layer_fwd_kernel's: 32-row tiles of one slot, one wave per tile, both
//  lc routes, rows that do not exist load nothing and store nothing.
//  The two taps' filter | gate weights are 2W x 2W floats (256 KiB at 128), so the output channels are walked in W / 32 blocks of 32:
//  for block c
//      pre_f, pre_g [32 x 32] = X[t-d] W0[:, c] + X[t] W1[:, c] + lc term       B operands: the block's slice [step][lane][filter, gate] in LDS
//      z_c = tanh(pre_f + bias + gc) * sigmoid(pre_g + bias + gc)               -> ZC, and through the wave's 32 x 36 LDS patch as A operand
//      acc[o] += z_c Wd[32c .. 32c+31, 32o .. 32o+31]   for all W / 32 output blocks o (W / 2 accumulator registers)
//  and x_next = X[t] + acc + bd at the end.  A operands (W / 2 registers per tap) are not held: every block reads the tile's rows
//  again (L1 / L2 hits).  At 64 all slices (64 KiB, staged 104 KiB) stay in LDS and the waves run free of each other; at 128 one slice
//  (64 KiB, staged 84 KiB) is resident at a time, so the eight waves of a workgroup take eight tiles in step: two barriers per block,
//  ~1e3 cycles of slice load against ~3e4 cycles of MFMA.  All addresses are 64-bit.
// ===================================================================================================================
template <int W, bool FUSED>
__global__ void __launch_bounds__(512) sc_layer_wide_fwd_kernel(ScLayerArgs a)
{
    constexpr int NB = W / 32;                               // channel blocks
    constexpr int W2 = 2 * W;
    constexpr int TAP = W / 2;                               // MFMA steps per tap (k = W)
    constexpr int STEPS = 2 * TAP + (FUSED ? 0 : 4 * kScLcSteps);
    constexpr bool RES = W == 64;                            // every slice resident
    constexpr int NSL = RES ? NB : 1;
    __shared__ __attribute__((aligned(16))) float bt[NSL * STEPS * 128];       // [slice][step][lane][filter, gate]
    __shared__ float bdt[NSL * NB * 16 * 64];                                   // dense: [slice][out block][step][lane]
    __shared__ __attribute__((aligned(16))) float cts[FUSED ? 4 * 512 : 4];    // ctab (hop <= 512)
    __shared__ __attribute__((aligned(16))) float zt[8][32 * 36];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 31, hh = lane >> 5;
    if (FUSED) for (int e = threadIdx.x; e < a.hop * 4; e += 512) cts[e] = a.ctab[e];
    // slice c of the weights -> LDS slot `slot` (step s, lane half h2 carries k = 8 (s >> 2) + 4 h2 + (s & 3) of its operand)
    auto load_slice = [&](int c, int slot) {
        float* bs = bt + slot * STEPS * 128;
        for (int e = threadIdx.x; e < STEPS * 64; e += 512) {
            const int s = e >> 6, l = e & 63, nn = l & 31, h2 = l >> 5;
            const float* Wp; int ij;
            if (s < TAP) { Wp = a.W0; ij = s; } else if (s < 2 * TAP) { Wp = a.W1; ij = s - TAP; } else { Wp = a.Wlc; ij = s - 2 * TAP; }
            const int k = 8 * (ij >> 2) + 4 * h2 + (ij & 3);
            bs[e * 2] = Wp[k * W2 + c * 32 + nn]; bs[e * 2 + 1] = Wp[k * W2 + W + c * 32 + nn];
        }
        float* ds = bdt + slot * NB * 16 * 64;
        for (int e = threadIdx.x; e < NB * 16 * 64; e += 512) {
            const int ob = e >> 10, s = (e >> 6) & 15, l = e & 63;
            ds[e] = a.Wd[(c * 32 + 8 * (s >> 2) + 4 * (l >> 5) + (s & 3)) * W + ob * 32 + (l & 31)];
        }
    };
    if (RES) {
        for (int c = 0; c < NB; ++c) load_slice(c, c);
        __syncthreads();
    }
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int ntiles = a.slots * a.tpb, ngroups = (ntiles + 7) / 8;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {                // block-uniform: every wave meets every barrier
        const int tile = grp * 8 + wave;
        const int b = tile < ntiles ? tile / a.tpb : 0, t0 = (tile - b * a.tpb) * 32 + a.t_lo;
        const int Tb = tile < ntiles ? a.lens[b] - 1 : 0;     // the slot's rows: its last sample is a target only (idle slot: -1)
        const bool active = tile < ntiles && t0 < Tb;         // wave-uniform: else the whole tile lies behind the slot's end
        const int t = t0 + n;
        const bool ok = active && t < Tb && t >= a.o;
        const float* xr = a.X + ((long long)b * a.Tn + t) * W + 4 * hh;          // lane (row, hh) carries k = 8i + 4hh .. +3 of its row
        const float* ur = a.U + ((long long)b * a.T + (t - a.o)) * 80 + 4 * hh;
        f32x16 cd[NB];
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) cd[ob] = zero;
        for (int c = 0; c < NB; ++c) {
            if (!RES) {
                __syncthreads();                              // the waves have finished with the slice before
                load_slice(c, 0);
                __syncthreads();
            }
            if (!active) continue;
            const float* bs = bt + (RES ? c : 0) * STEPS * 128 + lane * 2;
            const float* ds = bdt + (RES ? c : 0) * NB * 16 * 64 + lane;
            f32x16 cf = zero, cg = zero;
            if (FUSED) {                                      // the lc term first: the accumulators start from it
                // rows of the tile: U row u = t - o; at most two frames per 32-row tile (hop >= 32).  fA < F: t0 < Tb <= T - 1.
                int u0 = t0 - a.o; u0 = u0 < 0 ? 0 : u0;
                const int fA = u0 / a.hop, fB = fA + 1 < a.F ? fA + 1 : fA;
                const int edge = (fA + 1) * a.hop;                               // first U row of frame fA + 1
                const float* qa = a.Q + (((long long)b * a.F + fA) * 4) * W2 + c * 32 + n;
                const float* qb = a.Q + (((long long)b * a.F + fB) * 4) * W2 + c * 32 + n;
                float qfa[4], qga[4], qfb[4], qgb[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { qfa[j] = qa[j * W2]; qga[j] = qa[j * W2 + W]; qfb[j] = qb[j * W2]; qgb[j] = qb[j * W2 + W]; }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int uu = t0 - a.o + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    uu = uu < 0 ? 0 : uu;                                         // rows below the layer's offset are discarded by the epilogue
                    const bool hi = uu >= edge;
                    int ph = uu - (hi ? edge : edge - a.hop);
                    ph = ph < a.hop ? ph : a.hop - 1;                             // (only rows past the window's end, discarded as well)
                    const f32x4t ct = *reinterpret_cast<const f32x4t*>(&cts[ph * 4]);
                    const float f0 = hi ? qfb[0] : qfa[0], f1 = hi ? qfb[1] : qfa[1], f2 = hi ? qfb[2] : qfa[2], f3 = hi ? qfb[3] : qfa[3];
                    const float g0 = hi ? qgb[0] : qga[0], g1 = hi ? qgb[1] : qga[1], g2 = hi ? qgb[2] : qga[2], g3 = hi ? qgb[3] : qga[3];
                    cf[r] = ((ct[0] * f0 + ct[1] * f1) + ct[2] * f2) + ct[3] * f3;
                    cg[r] = ((ct[0] * g0 + ct[1] * g1) + ct[2] * g2) + ct[3] * g3;
                }
            }
#pragma unroll 2
            for (int i = 0; i < W / 8; ++i) {
                const f32x4t x0 = sc_ld4(xr - (long long)a.d * W + 8 * i, ok);   // t - d >= off[l]: a row of the layer's input
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x2t w = *reinterpret_cast<const f32x2t*>(&bs[(4 * i + j) * 128]);
                    cf = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[j], w[0], cf, 0, 0, 0);
                    cg = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[j], w[1], cg, 0, 0, 0);
                }
            }
#pragma unroll 2
            for (int i = 0; i < W / 8; ++i) {
                const f32x4t x1 = sc_ld4(xr + 8 * i, ok);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x2t w = *reinterpret_cast<const f32x2t*>(&bs[(TAP + 4 * i + j) * 128]);
                    cf = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[j], w[0], cf, 0, 0, 0);
                    cg = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[j], w[1], cg, 0, 0, 0);
                }
            }
            if (!FUSED) {
#pragma unroll 2
                for (int i = 0; i < kScLcSteps; ++i) {
                    const f32x4t u = sc_ld4(ur + 8 * i, ok);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x2t w = *reinterpret_cast<const f32x2t*>(&bs[(2 * TAP + 4 * i + j) * 128]);
                        cf = __builtin_amdgcn_mfma_f32_32x32x2f32(u[j], w[0], cf, 0, 0, 0);
                        cg = __builtin_amdgcn_mfma_f32_32x32x2f32(u[j], w[1], cg, 0, 0, 0);
                    }
                }
            }
            // ---- gated unit; rows that do not exist give z = 0 (a select, not a product: whatever their accumulators hold)
            const int ch = c * 32 + n;
            const float vbf = a.bf ? a.bf[ch] : 0.0f, vbg = a.bg ? a.bg[ch] : 0.0f;
            const float gcf = a.gcp ? a.gcp[b * W2 + ch] : 0.0f, gcg = a.gcp ? a.gcp[b * W2 + W + ch] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = (r & 3) + 8 * (r >> 2) + 4 * hh, tr = t0 + rl;
                const bool valid = tr < Tb && tr >= a.o;
                const float th = sc_tanh_fast((cf[r] + vbf) + gcf), sg = sc_sigmoid_fast((cg[r] + vbg) + gcg);
                const float z = valid ? th * sg : 0.0f;
                if (valid && tr >= a.cut) a.ZC[((long long)b * a.ow + (tr - a.cut)) * a.ldz + ch] = z;     // model.py:94-96: the last len_b - rf rows
                zt[wave][rl * 36 + n] = z;
            }
            // ---- dense 1x1: this block of z as A operand (row layout) back from the wave's LDS patch, into every output block
            {
                const float* zr = &zt[wave][n * 36 + 4 * hh];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4t q = *reinterpret_cast<const f32x4t*>(zr + 8 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int ob = 0; ob < NB; ++ob)
                            cd[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(q[j], ds[(ob * 16 + 4 * i + j) * 64], cd[ob], 0, 0, 0);
                }
            }
        }
        if (!active) continue;
        // ---- residual: x_next = X[t] + z Wd + bd in the output (C) layout: lane = channel, register r = row (r&3) + 8(r>>2) + 4hh
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) {
            const float vbd = a.bd ? a.bd[ob * 32 + n] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tr = t0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (tr < Tb && tr >= a.o) {
                    const long long at = ((long long)b * a.Tn + tr) * W + ob * 32 + n;
                    a.XN[at] = (a.X[at] + cd[ob][r]) + vbd;
                }
            }
        }
    }
}

// ---- per-row loss terms --------------------------------------------------------------------------------------------
// mixture.py:27-81 discretized_mix_logistic_loss(num_class=2**16, reduce=False), one row: the branch structure of the training step's
// tr_mol_row (edge branches at -0.999 / +0.999, cdf_delta > 1e-5, the log-scale clamp at log(1e-14)), forward only.
// NR > 0: the number of mixtures as a compile-time constant (the per-mixture terms stay in registers)
__device__ __forceinline__ float sc_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sc_sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
template <int NR>
__device__ __forceinline__ float sc_mol_row(const float* yr, float tgt, int nr_)
{
    const int nr = NR > 0 ? NR : nr_;
    constexpr int CAP = NR > 0 ? NR : 32;
    const float lsmin = -32.23619130191664f, h = 1.0f / 65535.0f, logc = logf(65535.0f / 2.0f);
    float lm = -3.0e38f;
#pragma unroll
    for (int i = 0; i < nr; ++i) lm = fmaxf(lm, yr[i]);
    float se = 0.0f;
#pragma unroll
    for (int i = 0; i < nr; ++i) se += expf(yr[i] - lm);
    const float lse_logit = lm + logf(se);
    float a[CAP];
    float amax = -3.0e38f;
#pragma unroll
    for (int i = 0; i < nr; ++i) {
        const float mu = yr[nr + i], s = fmaxf(yr[2 * nr + i], lsmin);
        const float cen = tgt - mu, inv = expf(-s);
        const float plus = inv * (cen + h), mn = inv * (cen - h), mid = inv * cen;
        const float delta = sc_sigm(plus) - sc_sigm(mn);
        float lp;
        if (tgt < -0.999f) lp = plus - sc_softplus(plus);
        else if (tgt > 0.999f) lp = -sc_softplus(mn);
        else if (delta > 1e-5f) lp = logf(fmaxf(delta, 1e-12f));
        else lp = mid - s - 2.0f * sc_softplus(mid) - logc;
        a[i] = lp + (yr[i] - lse_logit);
        amax = fmaxf(amax, a[i]);
    }
    float sa = 0.0f;
#pragma unroll
    for (int i = 0; i < nr; ++i) sa += expf(a[i] - amax);
    return -(amax + logf(sa));
}
// one thread per (slot, p): nll[slot][p] for p < len - rf (target audio[slot][p + rf]), 0 for the positions the slot does not have
template <int NR>
__global__ __launch_bounds__(256) void sc_mol_nll_kernel(const float* y, const float* audio, const int32_t* lens, int slots, int T, int ow, int rf, int nr, float* nll)
{
    GRID_STRIDE(r, (long long)slots * ow) {
        const int p = (int)(r % ow), b = (int)(r / ow);
        float v = 0.0f;
        if (p < lens[b] - rf) v = sc_mol_row<NR>(y + r * 3 * nr, audio[(long long)b * T + p + rf], nr);
        nll[r] = v;
    }
}
// model.py:293-296 softmax_cross_entropy_with_logits_v2(one-hot target), unreduced; one wave per row of Q logits (tr_softmax_ce_kernel's passes)
__global__ __launch_bounds__(256) void sc_softmax_nll_kernel(const float* y, const int32_t* q, const int32_t* lens, int slots, int T, int ow, int rf, int Q, float* nll)
{
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)slots * ow;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * 4) {
        const int p = (int)(r % ow), b = (int)(r / ow);
        if (p >= lens[b] - rf) { if (lane == 0) nll[r] = 0.0f; continue; }                  // wave-uniform
        const int tgt = q[(long long)b * T + p + rf];
        const float* yr = y + r * Q;
        float m = -3.0e38f;
        for (int i = lane; i < Q; i += 64) m = fmaxf(m, yr[i]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float se = 0.0f;
        for (int i = lane; i < Q; i += 64) se += expf(yr[i] - m);
        for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
        if (lane == 0) nll[r] = (m + logf(se)) - yr[tgt];
    }
}

// ---- (sum, count) of the kept positions: float64, one workgroup, a fixed order (thread i takes columns from + i, from + i + 1024, ...
// of slot 0, then of slot 1, ...; then a fixed tree) -- two runs give the same bits.  Up to 64 slots per launch; a later launch of the
// same call adds to what the earlier ones left (the launches of a stream run in order).
struct ScKeep { int from[64], to[64]; };
__global__ __launch_bounds__(1024) void sc_reduce_kernel(const float* nll, ScKeep k, int nslot, int width, int first, double* out)
{
    double s = 0.0;
    long long cnt = 0;
    for (int b = 0; b < nslot; ++b) {
        const float* row = nll + (long long)b * width;
        for (int p = k.from[b] + (int)threadIdx.x; p < k.to[b]; p += 1024) s += (double)row[p];
        cnt += k.to[b] - k.from[b];
    }
    __shared__ double sh[1024];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (first ? 0.0 : out[0]) + sh[0];
        out[1] = (first ? 0.0 : out[1]) + (double)cnt;
    }
}

// ---------------------------------------------------------------------------------------------------------------
//  host
// ---------------------------------------------------------------------------------------------------------------
// The workspace carve, each piece rounded up to 64 floats: create runs it on a null base for the SIZE, score_windows for the pointers.
// Nothing here grows with the utterances: it is (slots, window) activations of TWO layers, the stacked skip input and the head.
struct ScoreCarve {
    float* ups[5]; long long upT[5];
    float *xunf; int32_t* qin; int32_t* lens;
    float *XA, *XB, *ZC, *SK, *C1, *Y, *emb, *GCP, *WV, *WS, *bsum, *ctab, *melsh, *Qall;
    long long vstride, q_ls;
    long long o_ZC, o_Y;                                     // where ZC and Y start, in floats from the base (twv_wavenet_score_view)
};
static long long sc_carve(const WavenetGraph* h, float* base, ScoreCarve& c)
{
    const twv_wavenet_dims& d = h->d;
    const int B = h->rows, T = h->T, Tn = h->Tn, NL = h->NL, S = h->S, O = h->O, L = h->L, G = h->G, ow = h->ow;
    const long long Rr = (long long)B * Tn, RT = (long long)B * T, RO = (long long)B * ow;
    const bool fused = wavenet_route(*h).fused_lc;
    long long used = 0;
    auto take = [&](long long n) { float* p = base ? base + used : nullptr; used += (n + 63) / 64 * 64; return p; };
    c.upT[0] = h->F;
    for (int i = 0; i < d.n_upsample; ++i) c.upT[i + 1] = c.upT[i] * d.upsample_factor[i];
    c.ups[0] = nullptr;                                      // (the caller's mel frames)
    for (int i = 1; i <= d.n_upsample; ++i) c.ups[i] = take(fused ? 0 : (long long)B * c.upT[i] * L);
    c.xunf = take(d.scalar_input ? Rr * h->ifw : 0);
    c.qin = reinterpret_cast<int32_t*>(take(d.scalar_input ? 0 : RT));
    c.lens = reinterpret_cast<int32_t*>(take(B));
    const int R = h->R, D = h->D;                            // the width (R == D)
    c.XA = take(Rr * R); c.XB = take(Rr * R);                // the layers' activations ping-pong
    const int ZW = NL * D;                                   // stacked skip input: ZC[(b,p)][l*D + j]
    c.o_ZC = used; c.ZC = take(RO * ZW);
    c.SK = take(RO * S); c.C1 = take(RO * S);
    c.o_Y = used; c.Y = take(RO * O);
    c.emb = take((long long)B * G);
    c.GCP = take((long long)B * 2 * D * NL);
    c.vstride = 2LL * D * (2 * R + L + G);
    c.WV = take(c.vstride * NL); c.WS = take((long long)ZW * S);       // weight views (tr_views_kernel)
    c.bsum = take(S);
    c.ctab = take(fused ? 4LL * 512 : 0);
    c.melsh = take(fused ? (long long)B * h->F * 4 * L : 0);
    c.q_ls = (long long)B * h->F * 4 * 2 * D;
    c.Qall = take(fused ? (c.q_ls + 64) * NL : 0);
    return used;
}

extern "C" int twv_wavenet_score_create(const twv_wavenet_dims* dims, int slots, int window_samples, twv_wavenet_scorer** out)
{
    if (!out) return twv_fail(TWV_E_INVALID, "bad argument");
    twv_wavenet_scorer* h = new twv_wavenet_scorer();
    const int rc = wavenet_graph_init(h->g, dims, slots, window_samples, "scoring", 128);
    if (rc) { delete h; return rc; }
    h->blas = nullptr;
    ScoreCarve sizes;
    h->carve_floats = sc_carve(&h->g, nullptr, sizes);
    const WavenetRoute r = wavenet_route(h->g);
    h->route = wavenet_route_label(r, r.skinny ? "skinny" : "gemm") + " width=" + std::to_string(h->g.R) + " carve_floats=" + std::to_string(h->carve_floats);
    *out = h;
    return TWV_OK;
}
extern "C" void twv_wavenet_score_destroy(twv_wavenet_scorer* h)
{
    if (h && h->blas) rocblas_destroy_handle(h->blas);
    delete h;
}
extern "C" size_t twv_wavenet_score_workspace_bytes(const twv_wavenet_scorer* h) { return h ? (size_t)h->carve_floats * 4 : 0; }
extern "C" int twv_wavenet_score_output_width(const twv_wavenet_scorer* h) { return h ? h->g.ow : 0; }
extern "C" const char* twv_wavenet_score_route(const twv_wavenet_scorer* h) { return h ? h->route.c_str() : ""; }
extern "C" int twv_wavenet_score_view(const twv_wavenet_scorer* h, const char* name, long long* offset_floats, long long* rows, long long* cols)
{
    if (!h || !name || !offset_floats || !rows || !cols) return twv_fail(TWV_E_INVALID, "null argument");
    ScoreCarve cv;
    sc_carve(&h->g, nullptr, cv);
    const std::string nm(name);
    *rows = (long long)h->g.rows * h->g.ow;
    if (nm == "zc") { *offset_floats = cv.o_ZC; *cols = (long long)h->g.NL * h->g.D; }
    else if (nm == "y") { *offset_floats = cv.o_Y; *cols = h->g.O; }
    else return twv_fail(TWV_E_INVALID, "twv_wavenet_score_view: unknown array '" + nm + "' (zc, y)");
    return TWV_OK;
}

extern "C" int twv_wavenet_score_windows(twv_wavenet_scorer* h, const float* params, const float* audio, const float* lc, const int32_t* gc_ids,
                                         const int32_t* lengths_host, void* workspace, float* nll, void* stream)
{
    if (!h || !params || !audio || !lc || !gc_ids || !lengths_host || !workspace || !nll) return twv_fail(TWV_E_INVALID, "null argument");
    const WavenetGraph& g = h->g;
    const twv_wavenet_dims& d = g.d;
    const int B = g.rows, T = g.T, Tn = g.Tn, NL = g.NL, O = g.O, ow = g.ow, rf = g.rf, F = g.F;
    for (int b = 0; b < B; ++b) {
        const int n = lengths_host[b];
        if (n != 0 && (n < 0 || n > T || n % g.hop || n <= rf))
            return twv_fail(TWV_E_INVALID, "slot " + std::to_string(b) + ": length " + std::to_string(n) + " must be 0 (idle) or a multiple of the hop size " +
                                           std::to_string(g.hop) + " in (" + std::to_string(rf) + ", " + std::to_string(T) + "]");
    }
    ScoreCarve cv;
    if (sc_carve(&g, (float*)workspace, cv) != h->carve_floats)
        return twv_fail(TWV_E_INVALID, "internal: the workspace carve does not match the size twv_wavenet_score_create computed");
    hipStream_t st = (hipStream_t)stream;
    if (!h->blas) BLASCHK(rocblas_create_handle(&h->blas));
    BLASCHK(rocblas_set_stream(h->blas, st));
    BLASCHK(rocblas_set_pointer_mode(h->blas, rocblas_pointer_mode_host));
    const WavenetRoute route = wavenet_route(g);
    const long long RO = (long long)B * ow;
    const bool ub = d.use_biases != 0;
    const float* P = params;
    const int R = g.R, ZW = NL * g.D;
    const long long vstride = cv.vstride, q_ls = cv.q_ls;
    HIPCHK(hipMemcpyAsync(cv.lens, lengths_host, (size_t)B * 4, hipMemcpyHostToDevice, st));   // (pageable source: staged before the call returns)
    // ================= front: the training step's, on all slots x window rows =================
    WavenetFwdBufs fb;
    fb.ups[0] = const_cast<float*>(lc);
    for (int i = 1; i < 5; ++i) fb.ups[i] = cv.ups[i];
    fb.upT = cv.upT; fb.xunf = cv.xunf; fb.qin = cv.qin;
    fb.X0 = cv.XA; fb.emb = cv.emb; fb.GCP = cv.GCP; fb.WV = cv.WV; fb.WS = cv.WS; fb.ctab = cv.ctab; fb.melsh = cv.melsh; fb.Qall = cv.Qall;
    fb.vstride = vstride; fb.q_ls = q_ls;
    fb.ZC = cv.ZC; fb.SK = cv.SK; fb.C1 = cv.C1; fb.Y = cv.Y; fb.bsum = cv.bsum;
    if (int rc = wavenet_forward_front(g, P, audio, gc_ids, fb, h->blas, st)) return rc;
    const float* U = fb.ups[d.n_upsample];
    float* X[2] = {cv.XA, cv.XB};
    // ================= the residual stack: one forward-only kernel per layer =================
    for (int l = 0; l < NL; ++l) {
        const float* Lp = P + g.c_layer0 + (long long)l * g.c_lstride;
        const float* Wv = cv.WV + l * vstride;
        ScLayerArgs fa;
        fa.X = X[l & 1]; fa.XN = X[(l + 1) & 1]; fa.U = U; fa.gcp = cv.GCP + (long long)l * B * 2 * R;
        fa.W0 = Wv; fa.W1 = Wv + R * 2 * R; fa.Wlc = Wv + 2 * R * 2 * R; fa.Wd = Lp + g.lo.wd;
        fa.bf = ub ? Lp + g.lo.bf : nullptr; fa.bg = ub ? Lp + g.lo.bg : nullptr; fa.bd = ub ? Lp + g.lo.bd : nullptr;
        fa.ZC = cv.ZC + l * R; fa.lens = cv.lens;
        fa.slots = B; fa.T = T; fa.Tn = Tn; fa.d = d.dilations[l]; fa.o = g.off[l + 1]; fa.cut = rf - 1; fa.ow = ow; fa.ldz = ZW;
        fa.t_lo = (fa.o / 32) * 32;                          // whole tiles in front of the layer's offset hold no row: not walked
        fa.tpb = (Tn + 31) / 32 - fa.t_lo / 32;
        fa.Q = cv.Qall + l * (q_ls + 64); fa.ctab = cv.ctab; fa.hop = g.hop; fa.F = F;
        const int ntiles = B * fa.tpb;
        int nwg = (ntiles + 7) / 8; nwg = nwg > 256 ? 256 : nwg;     // one workgroup (8 waves, 2 per SIMD) per CU, each wave walks its tiles
        if (R == 32) {
            if (route.fused_lc) hipLaunchKernelGGL(sc_layer_fwd_kernel<true>, dim3(nwg), dim3(512), 0, st, fa);
            else hipLaunchKernelGGL(sc_layer_fwd_kernel<false>, dim3(nwg), dim3(512), 0, st, fa);
        } else if (R == 64) {                                 // (nwg: one workgroup per group of eight tiles, as above)
            if (route.fused_lc) hipLaunchKernelGGL((sc_layer_wide_fwd_kernel<64, true>), dim3(nwg), dim3(512), 0, st, fa);
            else hipLaunchKernelGGL((sc_layer_wide_fwd_kernel<64, false>), dim3(nwg), dim3(512), 0, st, fa);
        } else {
            if (route.fused_lc) hipLaunchKernelGGL((sc_layer_wide_fwd_kernel<128, true>), dim3(nwg), dim3(512), 0, st, fa);
            else hipLaunchKernelGGL((sc_layer_wide_fwd_kernel<128, false>), dim3(nwg), dim3(512), 0, st, fa);
        }
    }
    // ================= head: the training step's (model.py:150-165), over all slots x ow rows =================
    // the rows a slot does not have hold whatever the workspace held; every row is a function of itself only, and the loss kernels
    // below write those positions as 0.  conv1d_1's bias + relu pass is skipped whenever conv1d_2 is the skinny kernel.
    if (int rc = wavenet_forward_head(g, P, fb, route.skinny, route.skinny, h->blas, st)) return rc;
    // ================= per-row loss terms =================
#define K1(kern, n, ...) hipLaunchKernelGGL(kern, dim3(tg(n)), dim3(256), 0, st, __VA_ARGS__)
    if (route.loss == WG_LOSS_MOL10) K1(sc_mol_nll_kernel<10>, RO, cv.Y, audio, cv.lens, B, T, ow, rf, O / 3, nll);
    else if (route.loss == WG_LOSS_MOLN) K1(sc_mol_nll_kernel<0>, RO, cv.Y, audio, cv.lens, B, T, ow, rf, O / 3, nll);
    else hipLaunchKernelGGL(sc_softmax_nll_kernel, dim3(tg(RO * 64)), dim3(256), 0, st, cv.Y, cv.qin, cv.lens, B, T, ow, rf, O, nll);
#undef K1
    HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_wavenet_score_reduce(const float* nll, const int32_t* keep_from_host, const int32_t* keep_to_host, int slots, int width,
                                        double* out_double2, void* stream)
{
    if (!nll || !keep_from_host || !keep_to_host || !out_double2 || slots < 1 || width < 1) return twv_fail(TWV_E_INVALID, "bad argument");
    for (int b = 0; b < slots; ++b)
        if (keep_from_host[b] < 0 || keep_from_host[b] > keep_to_host[b] || keep_to_host[b] > width)
            return twv_fail(TWV_E_INVALID, "slot " + std::to_string(b) + ": kept columns must satisfy 0 <= from <= to <= width");
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < slots; b0 += 64) {
        ScKeep k;
        const int n = slots - b0 < 64 ? slots - b0 : 64;
        for (int i = 0; i < 64; ++i) { k.from[i] = i < n ? keep_from_host[b0 + i] : 0; k.to[i] = i < n ? keep_to_host[b0 + i] : 0; }
        hipLaunchKernelGGL(sc_reduce_kernel, dim3(1), dim3(1024), 0, st, nll + (long long)b0 * width, k, n, width, b0 == 0 ? 1 : 0, out_double2);
    }
    HIPCHK(hipGetLastError());
    return TWV_OK;
}
