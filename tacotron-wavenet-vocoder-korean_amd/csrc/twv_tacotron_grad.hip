// Tacotron decoder gradients (gfx950): the vector-Jacobian product of the TEACHER-FORCED decoder.
//
//   d_mel  ->  the gradient of every decoder-side weight tensor (memory_layer/kernel .. decoder/output_projection_wrapper/bias)
//              + d_memory (the attention memory) + d_init (the initial states of the attention cell and the residual GRUs)
//
// Teacher forcing cuts the feedback through the fed frame (helpers.py:80-87), so the recurrence runs through the attention GRU state, the
// context, the monotonic alignment and the residual GRU states only; the decoder prenet and the output projection are products over all
// N * steps rows.  The pass is
//   (a) a recording forward: prenet rows, then tg_forward_kernel -- ONE workgroup per utterance, steps 0 .. steps-1, every step's gates,
//       states, p_choose / cumprod / cumsum / alignment, context and projection input written to a tape in the workspace;
//   (b) tg_backward_kernel, one workgroup per utterance again, steps-1 .. 0: transposed products with the recurrent weights, the GRU and
//       attention backward, pre-activation deltas written beside the tape, d_keys / d_memory accumulated by the thread that owns the element;
//   (c) every kernel / bias gradient as ONE product (rocBLAS, atomics off) or column sum of saved inputs against saved deltas.
// No workgroup waits for another one anywhere: no exchange areas, tickets or grid barriers, so the pass cannot deadlock; the price is that
// each utterance's workgroup re-reads the decoder weights from L2 every step.  No atomics: two runs give the same bits.  Whatever feeds the
// recurrence (prenet, keys, d_mel through the output projection) goes through row kernels -- the gradient passes' shared grad_rows_kernel
// (twv_tacotron_grad_common.hpp) and, for the transposed products, this file's tg_rows_nt_kernel -- whose summation order for a row
// does not depend on how many rows there are: an utterance's d_memory / d_init are the same bits alone and inside a batch.
// Dot products accumulate in float64 (the kernels wait on L2, not on the VALU); tape and deltas are float32.
#include "twv_tacotron_blob.hpp"
#include "twv_tacotron_grad_common.hpp"

namespace tg {       // (helper names such as wave_sum exist in other files of the library with other bodies)

using namespace tgrad;

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr float kTiny = 1.17549435e-38f;          // np.finfo(np.float32).tiny: safe_cumprod's lower clip
constexpr float kCpMin = 1e-10f;                   // monotonic_attention(mode='parallel'): clip_by_value(cumprod, 1e-10, 1)
// The attention kinds of the two recurrent kernels (a template parameter), named as the split inference decoder names them:
//   AK_MON    bah_mon_norm, bah_mon: sigmoid(score + score_bias) through monotonic_attention(mode='parallel')
//   AK_SOFT   bah_norm, bah: softmax over the valid positions of the Bahdanau score
//   AK_LUONG  luong, luong_scaled: softmax of g * (h . keys_j), no query layer
//   AK_LOC    loc_sen: softmax of v . tanh(keys_j + W_q h + (conv31(c) . L)_j + conv_b . L + b_a), c the cumulative alignments
enum { AK_MON = 0, AK_SOFT = 1, AK_LUONG = 2, AK_LOC = 3 };
constexpr int kLocTaps = 31, kLocHalf = 15, kLocFilters = 32;      // location_features_convolution: kernel_size 31, 'same', 32 filters

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline float clampf_(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// out[j] = bias[j] + sum_k in(k) * W[k * ld + j], j < ncols <= 512; in(k) = k < split ? a[k] : b[k - split] (LDS).  512 / ncols threads share
// a column (contiguous k ranges), their partials are added in range order.  `red`: 512 doubles of LDS.  Ends with a barrier.
// A real call, not inlined: the forward kernel has a dozen call sites (and hipcc's inliner does not survive them all in one kernel).
// Its pointers arrive generic; they are cast back to their address spaces (W: global, the vectors: LDS) so that the weight loads are
// global loads the wave can keep eight of in flight, not flat loads that wait for the LDS reads between them.  Same order of additions.
#define TG_GLB __attribute__((address_space(1)))
#define TG_LDS __attribute__((address_space(3)))
__device__ __attribute__((noinline)) void tg_gemv(const float* W_, int ld, int K, int ncols, const float* a_, int split, const float* b_, const float* bias,
                        double* red_, float* out_)
{
    const TG_GLB float* W = (const TG_GLB float*)W_;
    const TG_LDS float *a = (const TG_LDS float*)a_, *b = (const TG_LDS float*)b_;
    TG_LDS double* red = (TG_LDS double*)red_;
    TG_LDS float* out = (TG_LDS float*)out_;
    const int tid = threadIdx.x, parts = kThreads / ncols;
    if (tid < parts * ncols) {
        const int col = tid % ncols, part = tid / ncols;
        const int k0 = (int)((long long)K * part / parts), k1 = (int)((long long)K * (part + 1) / parts);
        double acc = 0.0;
        int k = k0;
        for (; k + 8 <= k1; k += 8) {
            float w[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) w[r] = W[(long long)(k + r) * ld + col];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float x = k + r < split ? a[k + r] : b[k + r - split];
                acc = fma((double)w[r], (double)x, acc);
            }
        }
        for (; k < k1; ++k) {
            const float x = k < split ? a[k] : b[k - split];
            acc = fma((double)W[(long long)k * ld + col], (double)x, acc);
        }
        red[tid] = acc;
    }
    __syncthreads();
    if (tid < ncols) {
        double s = bias ? (double)bias[tid] : 0.0;
        for (int p = 0; p < parts; ++p) s += red[p * ncols + tid];
        out[tid] = (float)s;
    }
    __syncthreads();
}

// out[k] = sum_j W[k * ld + j] * d[j], k < K (the product with the transposed kernel): a wave takes eight rows at a time, its lanes stride
// over the columns.  d, out: LDS.  Ends with a barrier.
__device__ void tg_gemvT(const float* __restrict__ W, int ld, int K, int ncols, const float* d, float* out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int kRows = 8;      // rows whose loads a wave has in flight
    for (int k0 = w * kRows; k0 < K; k0 += kWaves * kRows) {
        double acc[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
        for (int j = lane; j < ncols; j += 64) {
            float wr[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) wr[r] = W[(long long)min(k0 + r, K - 1) * ld + j];
            const double dj = (double)d[j];
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] = fma((double)wr[r], dj, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const double s = wave_sum(acc[r]);
            if (lane == 0 && k0 + r < K) out[k0 + r] = (float)s;
        }
    }
    __syncthreads();
}

// in-place cumulative sum of a[0 .. T) in LDS by wave 0 (T <= 1024: at most 16 elements a lane), forward or from the end, inclusive or
// exclusive; float64 inside.  Called by every thread; ends with a barrier.
template <bool REV, bool EXCL>
__device__ void tg_scan(float* a, int T)
{
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x, chunk = (T + 63) / 64, b = lane * chunk, e = min(T, b + chunk);
        double loc = 0.0;
        for (int i = b; i < e; ++i) loc += (double)a[REV ? T - 1 - i : i];
        double inc = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        double run = inc - loc;
        for (int i = b; i < e; ++i) {
            const int j = REV ? T - 1 - i : i;
            const double x = (double)a[j];
            if (EXCL) { a[j] = (float)run; run += x; }
            else { run += x; a[j] = (float)run; }
        }
    }
    __syncthreads();
}

struct TgArgs {
    const float *blob, *memory, *init, *keys;
    const int32_t* lengths;
    TacoDecoderBlobCore w;
    int N, T, steps, D1, ENC, A, AS, DR, L, norm;
    // tape (row = n * steps + t)
    float *P, *XA, *GA, *XC, *QB, *PCH, *CP, *S, *AL, *XR[4], *GR[4], *YF;
    // backward
    const float* dYF;
    float *DAg, *DAc, *DQ, *DY0, *DRg[4], *DRc[4], *DP, *dkeys, *dmem, *dinit, *pv, *pb, *psb;
};
// The arguments of the AK_LOC instantiations alone (every other kind takes TgArgs as it always was).  CUM: the cumulative alignments a
// step reads, on the tape; F: the combined filter (31 x A) and, behind it, the combined bias (A) -- tg_loc_derive_kernel; GJ (T x A an
// utterance): a step's g_ja; U (T x 32 an utterance): a step's sum_a g_ja F[tap][a]; pF (31 x A doubles an utterance): the utterance's dF
struct TgLocArgs : TgArgs {
    float *CUM, *F, *GJ, *U;
    double* pF;
};
template <int AK> struct TgArgsOf { using type = TgArgs; };
template <> struct TgArgsOf<AK_LOC> { using type = TgLocArgs; };

// LDS of the two recurrent kernels, in floats: one carve for the kernel and for the host's launch size.  lf (the combined filter), cum
// (the cumulative alignments between 16 zeros on either side) and dcum (the cotangent on them) exist for AK_LOC only.
struct TgFwdLds { int red, x, g, xc, qb, vh, xr, gr, dech, al, pc, cp, ss, lf, cum, total; };
__host__ __device__ inline TgFwdLds tg_fwd_lds(int T, int D1, int ENC, int A, int AS, int DR, int L, int ak)
{
    TgFwdLds c; Take<int> take; const int Tp = (T + 3) & ~3;
    c.red = take(2 * kThreads); c.x = take(D1 + ENC + 2 * AS); c.g = take(3 * AS); c.xc = take(AS + ENC); c.qb = take(A); c.vh = take(A);
    c.xr = take(3 * DR); c.gr = take(3 * DR); c.dech = take(L * DR); c.al = take(Tp); c.pc = take(Tp); c.cp = take(Tp); c.ss = take(Tp);
    c.lf = take(ak == AK_LOC ? kLocTaps * A : 0); c.cum = take(ak == AK_LOC ? Tp + 32 : 0);
    c.total = take.used;
    return c;
}
struct TgBwdLds { int acc, dha, dctx, ddech, dy, dhl, dcl, dgl, dxh, dxh2, dx, tmp, vh, qb, dq, wp, dal, t1, t2, de, lf, cum, dcum, total; };
__host__ __device__ inline TgBwdLds tg_bwd_lds(int T, int D1, int ENC, int A, int AS, int DR, int L, int ak)
{
    TgBwdLds c; Take<int> take; const int Tp = (T + 3) & ~3;
    const int U = AS > DR ? AS : DR, KX = (D1 + ENC + AS) > 2 * DR ? (D1 + ENC + AS) : 2 * DR;
    c.acc = take(4 * A);                           // two arrays of A doubles: the utterance's sums for attention_v-hat and attention_b
    c.dha = take(AS); c.dctx = take(ENC); c.ddech = take(L * DR); c.dy = take(DR); c.dhl = take(U); c.dcl = take(U); c.dgl = take(2 * U);
    c.dxh = take(KX); c.dxh2 = take(KX); c.dx = take(KX); c.tmp = take(AS + ENC); c.vh = take(A); c.qb = take(A); c.dq = take(A);
    c.wp = take(2 * kWaves * A); c.dal = take(Tp); c.t1 = take(Tp); c.t2 = take(Tp); c.de = take(Tp);
    c.lf = take(ak == AK_LOC ? kLocTaps * A : 0); c.cum = take(ak == AK_LOC ? Tp + 32 : 0); c.dcum = take(ak == AK_LOC ? Tp : 0);
    c.total = take.used;
    return c;
}

// v-hat = g * v / ||v|| (normalised score) or v; every wave computes the same value
__device__ void tg_vhat(const TgArgs& a, float* vh)
{
    const float* v = a.blob + a.w.av;
    const int lane = threadIdx.x & 63;
    double ss = 0.0;
    for (int i = lane; i < a.A; i += 64) ss += (double)v[i] * (double)v[i];
    ss = wave_sum(ss);
    const float nrm = (float)sqrt(ss), g = a.norm ? a.blob[a.w.ag] : 1.0f;
    for (int i = threadIdx.x; i < a.A; i += kThreads) vh[i] = a.norm ? g * v[i] / nrm : v[i];
    __syncthreads();
}

// alpha = softmax(e) over the positions below len (len >= 1), exactly 0 from len to T: the maximum shift, then ONE float64 sum in fixed
// order (a thread's positions ascending, the wave's butterfly, the eight waves in order).  e, al: LDS; red: 24 doubles of LDS scratch.
// Called by every thread; ends with a barrier.
__device__ void tg_softmax(const float* e, float* al, int len, int T, double* red)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* redf = reinterpret_cast<float*>(red);               // the waves' maxima: red[0 .. 4); their sums: red[8 .. 16)
    float m = -INFINITY;
    for (int j = tid; j < len; j += kThreads) m = fmaxf(m, e[j]);
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) redf[wv] = m;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) m = fmaxf(m, redf[w]);
    double s = 0.0;
    for (int j = tid; j < len; j += kThreads) { const float ex = expf(e[j] - m); al[j] = ex; s += (double)ex; }
    s = wave_sum(s);
    if (lane == 0) red[8 + wv] = s;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < kWaves; ++w) tot += red[8 + w];
    for (int j = tid; j < T; j += kThreads) al[j] = j < len ? (float)((double)al[j] / tot) : 0.0f;
    __syncthreads();
}

// the location term of loc_sen's score at position j, column i: sum_tap c[j + tap - 15] F[tap][i], taps ascending in float64.  The
// cumulative alignments lie in LDS between 16 zeros on either side (c[j] at index 16 + j); cumj points at index j, so cumj[tap + 1] is
// position j + tap - 15.  F: LDS.  One function for the forward and the backward, which recomputes the tanh: the same bits.
__device__ inline float tg_loc_term(const float* cumj, const float* F, int A, int i)
{
    double s = 0.0;
#pragma unroll
    for (int tap = 0; tap < kLocTaps; ++tap) s = fma((double)cumj[tap + 1], (double)F[tap * A + i], s);
    return (float)s;
}

// AK_LOC, once a pass: the convolution and the dense layer behind it have no nonlinearity between them, so the recurrence works with
// F[tap][a] = sum_c K[tap][c] L[c][a] and f_b[a] = sum_c conv_b[c] L[c][a] + b_a[a] (float64, c ascending); out = F (31 x A), then f_b (A)
__global__ void tg_loc_derive_kernel(const float* blob, TacoDecoderBlob w, int A, float* out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (kLocTaps + 1) * A) return;
    const int tap = idx / A, i = idx - tap * A;
    const float* Lk = blob + w.lcL;
    const float* row = tap < kLocTaps ? blob + w.lcK + (long long)tap * kLocFilters : blob + w.lcb;
    double s = 0.0;
    for (int cc = 0; cc < kLocFilters; ++cc) s = fma((double)row[cc], (double)Lk[(long long)cc * A + i], s);
    if (tap == kLocTaps) s += (double)blob[w.ab + i];
    out[idx] = (float)s;
}

// (a) the recording forward: blockIdx.x = utterance
template <int AK>
__global__ void __launch_bounds__(kThreads) tg_forward_kernel(typename TgArgsOf<AK>::type a)
{
    extern __shared__ float lds[];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = a.T, D1 = a.D1, ENC = a.ENC, A = a.A, AS = a.AS, DR = a.DR, L = a.L, ain = D1 + ENC, XW = ain + 2 * AS;
    const int len = min(max(a.lengths[n], 0), T);
    const TgFwdLds c = tg_fwd_lds(T, D1, ENC, A, AS, DR, L, AK);
    double* red = reinterpret_cast<double*>(lds + c.red);
    float *x = lds + c.x, *g = lds + c.g, *xc = lds + c.xc, *qb = lds + c.qb, *vh = lds + c.vh, *xr = lds + c.xr, *gr = lds + c.gr,
          *dech = lds + c.dech, *al = lds + c.al, *pc = lds + c.pc, *cp = lds + c.cp, *ss = lds + c.ss;
    const float* B = a.blob;
    const float* init = a.init + (long long)n * (AS + L * DR);
    const float* mem = a.memory + (long long)n * T * ENC;
    const float* keys = a.keys + (long long)n * T * A;
    float sb = 0.0f, lg = 1.0f;                                                       // score bias (AK_MON); Luong's scale
    if constexpr (AK == AK_MON) sb = B[a.w.asb];
    if constexpr (AK == AK_LUONG) lg = a.norm ? B[a.w.ag] : 1.0f;
    if constexpr (AK != AK_LUONG) tg_vhat(a, vh);
    for (int i = tid; i < ENC; i += kThreads) x[D1 + i] = 0.0f;                      // AttentionWrapper.zero_state: attention = zeros
    for (int i = tid; i < AS; i += kThreads) x[ain + i] = init[i];
    for (int i = tid; i < L * DR; i += kThreads) dech[i] = init[AS + i];
    if constexpr (AK == AK_MON)
        for (int j = tid; j < T; j += kThreads) al[j] = j == 0 ? 1.0f : 0.0f;        // monotonic initial alignments: one_hot(0)
    // (the softmax kinds' initial alignments are zeros that nothing reads)
    if constexpr (AK == AK_LOC) {
        float *lf = lds + c.lf, *cum = lds + c.cum;
        for (int i = tid; i < kLocTaps * A; i += kThreads) lf[i] = a.F[i];
        for (int j = tid; j < ((T + 3) & ~3) + 32; j += kThreads) cum[j] = 0.0f;     // the state starts from zeros; zeros outside [0, T)
    }
    __syncthreads();
    for (int t = 0; t < a.steps; ++t) {
        const long long row = (long long)n * a.steps + t;
        for (int i = tid; i < D1; i += kThreads) x[i] = a.P[row * D1 + i];
        __syncthreads();
        // attention GRU on [prenet_t | context_{t-1}], state att_h
        tg_gemv(B + a.w.aWg, 2 * AS, ain + AS, 2 * AS, x, ain + AS, nullptr, B + a.w.abg, red, g);
        for (int i = tid; i < 2 * AS; i += kThreads) g[i] = sigmoidf_(g[i]);
        __syncthreads();
        for (int i = tid; i < AS; i += kThreads) x[ain + AS + i] = g[i] * x[ain + i];
        __syncthreads();
        tg_gemv(B + a.w.aWc, AS, ain + AS, AS, x, ain, x + ain + AS, B + a.w.abc, red, g + 2 * AS);
        for (int i = tid; i < AS; i += kThreads) g[2 * AS + i] = tanhf(g[2 * AS + i]);
        __syncthreads();
        for (int i = tid; i < XW; i += kThreads) a.XA[row * XW + i] = x[i];
        for (int i = tid; i < 3 * AS; i += kThreads) a.GA[row * 3 * AS + i] = g[i];
        for (int i = tid; i < AS; i += kThreads) { const float u = g[AS + i]; xc[i] = u * x[ain + i] + (1.0f - u) * g[2 * AS + i]; }
        __syncthreads();
        for (int i = tid; i < AS; i += kThreads) x[ain + i] = xc[i];
        if constexpr (AK == AK_MON) {
        // query layer (+ attention_b): the tanh argument is keys + qb
        tg_gemv(B + a.w.Wq, A, AS, A, xc, AS, nullptr, a.norm ? B + a.w.ab : nullptr, red, qb);
        for (int i = tid; i < A; i += kThreads) a.QB[row * A + i] = qb[i];
        // Bahdanau score, masked past the length (-inf -> p_choose 0), sigmoid
        for (int j = wv; j < T; j += kWaves) {
            float p = 0.0f;
            if (j < len) {
                double acc = 0.0;
                for (int i = lane; i < A; i += 64) acc += (double)(vh[i] * tanhf(keys[(long long)j * A + i] + qb[i]));
                p = sigmoidf_((float)wave_sum(acc) + sb);
            }
            if (lane == 0) pc[j] = p;
        }
        __syncthreads();
        // monotonic_attention(mode='parallel')
        for (int j = tid; j < T; j += kThreads) ss[j] = logf(clampf_(1.0f - pc[j], kTiny, 1.0f));
        __syncthreads();
        tg_scan<false, true>(ss, T);
        for (int j = tid; j < T; j += kThreads) { const float cpj = expf(ss[j]); cp[j] = cpj; ss[j] = al[j] / clampf_(cpj, kCpMin, 1.0f); }
        __syncthreads();
        tg_scan<false, false>(ss, T);
        for (int j = tid; j < T; j += kThreads) {
            const float v = pc[j] * cp[j] * ss[j];
            al[j] = v;
            a.PCH[row * T + j] = pc[j]; a.CP[row * T + j] = cp[j]; a.S[row * T + j] = ss[j]; a.AL[row * T + j] = v;
        }
        __syncthreads();
        } else {
        // the softmax kinds.  Query layer (AK_SOFT: + attention_b of the normalised score; AK_LOC: + f_b); Luong has none
        if constexpr (AK != AK_LUONG) {
            const float* qbias = a.norm ? B + a.w.ab : nullptr;
            if constexpr (AK == AK_LOC) qbias = a.F + kLocTaps * A;
            tg_gemv(B + a.w.Wq, A, AS, A, xc, AS, nullptr, qbias, red, qb);
            for (int i = tid; i < A; i += kThreads) a.QB[row * A + i] = qb[i];
        }
        // the score of the utterance's own positions (what lies past the length is masked with -inf: alignment exactly 0)
        for (int j = wv; j < len; j += kWaves) {
            double acc = 0.0;
            if constexpr (AK == AK_LUONG) {
                for (int i = lane; i < A; i += 64) acc = fma((double)xc[i], (double)keys[(long long)j * A + i], acc);
            } else if constexpr (AK == AK_LOC) {
                const float *lf = lds + c.lf, *cumj = lds + c.cum + j;
                for (int i = lane; i < A; i += 64)
                    acc += (double)(vh[i] * tanhf((keys[(long long)j * A + i] + qb[i]) + tg_loc_term(cumj, lf, A, i)));
            } else {
                for (int i = lane; i < A; i += 64) acc += (double)(vh[i] * tanhf(keys[(long long)j * A + i] + qb[i]));
            }
            const float e = (float)wave_sum(acc);
            if (lane == 0) pc[j] = AK == AK_LUONG ? lg * e : e;
        }
        __syncthreads();
        tg_softmax(pc, al, len, T, red);
        for (int j = tid; j < T; j += kThreads) {
            a.AL[row * T + j] = al[j];
            if constexpr (AK == AK_LOC) {                                            // the tape holds the c this step read; then c <- c + alpha
                float* cum = lds + c.cum + 16;
                a.CUM[row * T + j] = cum[j];
                cum[j] = cum[j] + al[j];
            }
        }
        __syncthreads();
        }
        // context over the utterance's own positions (memory is zero past the length)
        tg_gemv(mem, ENC, len, ENC, al, len, nullptr, nullptr, red, xc + AS);
        for (int i = tid; i < ENC; i += kThreads) x[D1 + i] = xc[AS + i];
        for (int i = tid; i < AS + ENC; i += kThreads) a.XC[row * (AS + ENC) + i] = xc[i];
        // cell_0 projection of [att_h | context], then the residual GRUs
        tg_gemv(B + a.w.cW, DR, AS + ENC, DR, xc, AS + ENC, nullptr, B + a.w.cb, red, xr);
        for (int l = 0; l < L; ++l) {
            for (int i = tid; i < DR; i += kThreads) xr[DR + i] = dech[l * DR + i];
            __syncthreads();
            tg_gemv(B + a.w.rWg[l], 2 * DR, 2 * DR, 2 * DR, xr, 2 * DR, nullptr, B + a.w.rbg[l], red, gr);
            for (int i = tid; i < 2 * DR; i += kThreads) gr[i] = sigmoidf_(gr[i]);
            __syncthreads();
            for (int i = tid; i < DR; i += kThreads) xr[2 * DR + i] = gr[i] * xr[DR + i];
            __syncthreads();
            tg_gemv(B + a.w.rWc[l], DR, 2 * DR, DR, xr, DR, xr + 2 * DR, B + a.w.rbc[l], red, gr + 2 * DR);
            for (int i = tid; i < DR; i += kThreads) gr[2 * DR + i] = tanhf(gr[2 * DR + i]);
            __syncthreads();
            for (int i = tid; i < 3 * DR; i += kThreads) { a.XR[l][row * 3 * DR + i] = xr[i]; a.GR[l][row * 3 * DR + i] = gr[i]; }
            for (int i = tid; i < DR; i += kThreads) { const float u = gr[DR + i]; dech[l * DR + i] = u * xr[DR + i] + (1.0f - u) * gr[2 * DR + i]; }
            __syncthreads();
            for (int i = tid; i < DR; i += kThreads) xr[i] += dech[l * DR + i];       // ResidualWrapper
            __syncthreads();
        }
        for (int i = tid; i < DR; i += kThreads) a.YF[row * DR + i] = xr[i];
        __syncthreads();
    }
}

// GRUCell backward for one row.  Xrow = [x (nin) | h (U) | r * h (U)], Grow = [r | u | c]; dh: in dL/dh', out dL/dh (LDS); dx (nin, LDS) is
// assigned; the pre-activation deltas go to dgrow (2U) and dcrow (U).  dcl (U), dgl (2U), dxh, dxh2 (nin + U): LDS scratch.
// Inlined by force: with one backward kernel the compiler inlined both calls by itself; with four instantiations it stops, and the
// monotonic kernel would no longer be the code it was.
__device__ __forceinline__ void tg_gru_bwd(const float* __restrict__ Wg, const float* __restrict__ Wc, int nin, int U, const float* __restrict__ Xrow,
                           const float* __restrict__ Grow, float* dh, float* dx, float* dgrow, float* dcrow, float* dcl, float* dgl,
                           float* dxh, float* dxh2)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < U; i += kThreads) {
        const float u = Grow[U + i], cc = Grow[2 * U + i], h = Xrow[nin + i], d = dh[i];
        const float dcp = d * (1.0f - u) * (1.0f - cc * cc);
        dcl[i] = dcp; dcrow[i] = dcp;
        dgl[U + i] = d * (h - cc) * u * (1.0f - u);
    }
    __syncthreads();
    tg_gemvT(Wc, U, nin + U, U, dcl, dxh);
    for (int i = tid; i < U; i += kThreads) {
        const float r = Grow[i], u = Grow[U + i], h = Xrow[nin + i], drh = dxh[nin + i];
        dgl[i] = drh * h * r * (1.0f - r);
        dh[i] = dh[i] * u + drh * r;
    }
    __syncthreads();
    for (int i = tid; i < 2 * U; i += kThreads) dgrow[i] = dgl[i];
    tg_gemvT(Wg, 2 * U, nin + U, 2 * U, dgl, dxh2);
    for (int i = tid; i < nin; i += kThreads) dx[i] = dxh[i] + dxh2[i];
    for (int i = tid; i < U; i += kThreads) dh[i] += dxh2[nin + i];
    __syncthreads();
}

// (b) backward through time: blockIdx.x = utterance
template <int AK>
__global__ void __launch_bounds__(kThreads) tg_backward_kernel(typename TgArgsOf<AK>::type a)
{
    extern __shared__ float lds[];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = a.T, D1 = a.D1, ENC = a.ENC, A = a.A, AS = a.AS, DR = a.DR, L = a.L, ain = D1 + ENC, XW = ain + 2 * AS;
    const int len = min(max(a.lengths[n], 0), T);
    const TgBwdLds c = tg_bwd_lds(T, D1, ENC, A, AS, DR, L, AK);
    double *accv = reinterpret_cast<double*>(lds + c.acc), *accb = accv + A;
    float *dha = lds + c.dha, *dctx = lds + c.dctx, *ddech = lds + c.ddech, *dy = lds + c.dy, *dhl = lds + c.dhl, *dcl = lds + c.dcl,
          *dgl = lds + c.dgl, *dxh = lds + c.dxh, *dxh2 = lds + c.dxh2, *dx = lds + c.dx, *tmp = lds + c.tmp, *vh = lds + c.vh, *qb = lds + c.qb,
          *dq = lds + c.dq, *wp = lds + c.wp, *dal = lds + c.dal, *t1 = lds + c.t1, *t2 = lds + c.t2, *de = lds + c.de;
    const float* B = a.blob;
    const float* mem = a.memory + (long long)n * T * ENC;
    const float* keys = a.keys + (long long)n * T * A;
    float* dmem = a.dmem + (long long)n * T * ENC;
    float* dkeys = a.dkeys + (long long)n * T * A;
    float lg = 1.0f;                                                                 // Luong's scale
    if constexpr (AK == AK_LUONG) lg = a.norm ? B[a.w.ag] : 1.0f;
    if constexpr (AK != AK_LUONG) tg_vhat(a, vh);
    if constexpr (AK == AK_LOC) {
        float *lf = lds + c.lf, *cum = lds + c.cum, *dcum = lds + c.dcum;
        for (int i = tid; i < kLocTaps * A; i += kThreads) lf[i] = a.F[i];
        for (int j = tid; j < ((T + 3) & ~3) + 32; j += kThreads) cum[j] = 0.0f;     // zeros outside [0, T)
        for (int j = tid; j < T; j += kThreads) dcum[j] = 0.0f;                      // nothing reads the state after the last step
    }
    for (int i = tid; i < T * ENC; i += kThreads) dmem[i] = 0.0f;
    for (int i = tid; i < T * A; i += kThreads) dkeys[i] = 0.0f;
    for (int i = tid; i < AS; i += kThreads) dha[i] = 0.0f;
    for (int i = tid; i < ENC; i += kThreads) dctx[i] = 0.0f;
    for (int i = tid; i < L * DR; i += kThreads) ddech[i] = 0.0f;
    for (int j = tid; j < T; j += kThreads) dal[j] = 0.0f;
    for (int i = tid; i < A; i += kThreads) { accv[i] = 0.0; accb[i] = 0.0; }
    double accsb = 0.0;                                                              // (thread 0's)
    __syncthreads();
    for (int t = a.steps - 1; t >= 0; --t) {
        const long long row = (long long)n * a.steps + t;
        // residual GRUs, last layer first: y_{l+1} = y_l + h'_l
        for (int i = tid; i < DR; i += kThreads) dy[i] = a.dYF[row * DR + i];
        __syncthreads();
        for (int l = L - 1; l >= 0; --l) {
            for (int i = tid; i < DR; i += kThreads) dhl[i] = dy[i] + ddech[l * DR + i];
            __syncthreads();
            tg_gru_bwd(B + a.w.rWg[l], B + a.w.rWc[l], DR, DR, a.XR[l] + row * 3 * DR, a.GR[l] + row * 3 * DR, dhl, dx,
                       a.DRg[l] + row * 2 * DR, a.DRc[l] + row * DR, dcl, dgl, dxh, dxh2);
            for (int i = tid; i < DR; i += kThreads) { ddech[l * DR + i] = dhl[i]; dy[i] += dx[i]; }
            __syncthreads();
        }
        // cell_0 projection of [att_h | context]
        for (int i = tid; i < DR; i += kThreads) a.DY0[row * DR + i] = dy[i];
        tg_gemvT(B + a.w.cW, DR, AS + ENC, DR, dy, tmp);
        for (int i = tid; i < AS; i += kThreads) dha[i] += tmp[i];
        for (int i = tid; i < ENC; i += kThreads) dctx[i] += tmp[AS + i];
        __syncthreads();
        // context = alignment . memory
        for (int j = wv; j < len; j += kWaves) {
            const float alj = a.AL[row * T + j];
            double acc = 0.0;
            for (int i = lane; i < ENC; i += 64) {
                acc = fma((double)dctx[i], (double)mem[(long long)j * ENC + i], acc);
                dmem[(long long)j * ENC + i] += alj * dctx[i];
            }
            acc = wave_sum(acc);
            if (lane == 0) {
                if constexpr (AK == AK_MON) dal[j] += (float)acc;                    // + what step t + 1 left for its alpha_prev
                else if constexpr (AK == AK_LOC) dal[j] = (float)acc + lds[c.dcum + j];   // + the cotangent on c_{t+1} = c_t + alpha_t
                else dal[j] = (float)acc;                                            // no gradient flows to the previous alignment
            }
        }
        __syncthreads();
        if constexpr (AK == AK_MON) {
        // monotonic attention: alpha = p * cp * s, s = cumsum(alpha_prev / clamp(cp)), cp = exp(exclusive cumsum(log(clamp(1 - p))))
        for (int j = tid; j < T; j += kThreads) {
            const float dA = dal[j], p = a.PCH[row * T + j], cpj = a.CP[row * T + j], s = a.S[row * T + j];
            t1[j] = dA * p * cpj;            // ds
            t2[j] = dA * p * s;              // dcp
            de[j] = dA * cpj * s;            // dp
        }
        __syncthreads();
        tg_scan<true, false>(t1, T);         // du_j = sum_{i >= j} ds_i
        for (int j = tid; j < T; j += kThreads) {
            const float cpj = a.CP[row * T + j], ct = clampf_(cpj, kCpMin, 1.0f), du = t1[j];
            const float aprev = t > 0 ? a.AL[(row - 1) * T + j] : (j == 0 ? 1.0f : 0.0f);
            dal[j] = du / ct;                // d alpha_prev: what step t - 1 starts from
            float dcp = t2[j];
            if (cpj >= kCpMin && cpj <= 1.0f) dcp -= du * aprev / (ct * ct);
            t2[j] = dcp * cpj;               // d (exclusive cumsum of the logs) at j
        }
        __syncthreads();
        tg_scan<true, true>(t2, T);          // dL_j = sum_{i > j}
        for (int j = tid; j < T; j += kThreads) {
            const float p = a.PCH[row * T + j], m = 1.0f - p;
            float dp = de[j];
            if (m >= kTiny && m <= 1.0f) dp -= t2[j] / m;
            de[j] = j < len ? dp * p * (1.0f - p) : 0.0f;
        }
        } else {
        // softmax: de_j = alpha_j (dalpha_j - sum_k alpha_k dalpha_k), the sum in float64 over the valid positions in fixed order.  An
        // utterance of one position has alpha = 1, the sum is dalpha itself and de is exactly 0.
        double s = 0.0;
        for (int j = tid; j < len; j += kThreads) s = fma((double)a.AL[row * T + j], (double)dal[j], s);
        s = wave_sum(s);
        double* rd = reinterpret_cast<double*>(wp);
        if (lane == 0) rd[wv] = s;
        __syncthreads();
        double tot = 0.0;
        for (int w = 0; w < kWaves; ++w) tot += rd[w];
        for (int j = tid; j < T; j += kThreads) de[j] = j < len ? (float)((double)a.AL[row * T + j] * ((double)dal[j] - tot)) : 0.0f;
        if constexpr (AK == AK_LOC)
            for (int j = tid; j < T; j += kThreads) lds[c.cum + 16 + j] = a.CUM[row * T + j];     // the c this step read
        }
        if constexpr (AK != AK_LUONG) {
        for (int i = tid; i < A; i += kThreads) qb[i] = a.QB[row * A + i];
        __syncthreads();
        // score_j = v-hat . tanh(keys_j + q + b) + score_bias    (AK_LOC: + the location term inside the tanh; no score bias but AK_MON's)
        {
            double aq[4] = {0.0, 0.0, 0.0, 0.0}, av[4] = {0.0, 0.0, 0.0, 0.0};      // attention_size <= 256: four columns a lane
            for (int j = wv; j < len; j += kWaves) {
                const float dej = de[j];
                float gj[4] = {0.0f, 0.0f, 0.0f, 0.0f};                              // (AK_LOC) g_ja of the lane's columns
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = lane + 64 * q;
                    if (i < A) {
                        float arg = keys[(long long)j * A + i] + qb[i];
                        if constexpr (AK == AK_LOC) arg = arg + tg_loc_term(lds + c.cum + j, lds + c.lf, A, i);
                        const float th = tanhf(arg);
                        const float gq = dej * vh[i] * (1.0f - th * th);
                        aq[q] += (double)gq; av[q] += (double)(dej * th);
                        dkeys[(long long)j * A + i] += gq;
                        if constexpr (AK == AK_LOC) { gj[q] = gq; a.GJ[((long long)n * T + j) * A + i] = gq; }
                    }
                }
                if constexpr (AK == AK_LOC) {
                    // U[j][tap] = sum_a g_ja F[tap][a]: what position j sends to the cotangent on c at j + tap - 15
                    const float* lf = lds + c.lf;
                    for (int tap = 0; tap < kLocTaps; ++tap) {
                        double u = 0.0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int i = lane + 64 * q;
                            if (i < A) u = fma((double)gj[q], (double)lf[tap * A + i], u);
                        }
                        u = wave_sum(u);
                        if (lane == 0) a.U[((long long)n * T + j) * 32 + tap] = (float)u;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = lane + 64 * q;
                if (i < A) { wp[wv * A + i] = (float)aq[q]; wp[(kWaves + wv) * A + i] = (float)av[q]; }
            }
        }
        __syncthreads();
        for (int i = tid; i < A; i += kThreads) {
            double sq = 0.0, sv = 0.0;
            for (int w = 0; w < kWaves; ++w) { sq += (double)wp[w * A + i]; sv += (double)wp[(kWaves + w) * A + i]; }
            dq[i] = (float)sq; a.DQ[row * A + i] = (float)sq;
            accb[i] += sq; accv[i] += sv;
        }
        if constexpr (AK == AK_MON)
            if (tid == 0) for (int j = 0; j < len; ++j) accsb += (double)de[j];
        if constexpr (AK == AK_LOC) {
            // (the barrier above has made this step's GJ and U, written by other waves of this workgroup, visible)
            // the cotangent on c_t: D_t[j] = D_{t+1}[j] + sum_tap U[j - tap + 15][tap], taps ascending, float64
            const float* U = a.U + (long long)n * T * 32;
            for (int j = tid; j < len; j += kThreads) {
                double s = (double)lds[c.dcum + j];
                for (int tap = 0; tap < kLocTaps; ++tap) {
                    const int jp = j - tap + kLocHalf;
                    if (jp >= 0 && jp < len) s += (double)U[(long long)jp * 32 + tap];
                }
                lds[c.dcum + j] = (float)s;
            }
            // dF[tap][a] += sum_j g_ja c[j + tap - 15]: each element has one owner thread, positions ascending, float64 across the steps
            const float* GJ = a.GJ + (long long)n * T * A;
            double* pF = a.pF + (long long)n * kLocTaps * A;
            for (int idx = tid; idx < kLocTaps * A; idx += kThreads) {
                const int tap = idx / A, i = idx - tap * A;
                double acc = t == a.steps - 1 ? 0.0 : pF[idx];
                for (int j = 0; j < len; ++j) acc = fma((double)GJ[(long long)j * A + i], (double)lds[c.cum + j + tap + 1], acc);
                pF[idx] = acc;
            }
        }
        __syncthreads();
        tg_gemvT(B + a.w.Wq, A, AS, A, dq, tmp);
        for (int i = tid; i < AS; i += kThreads) dhl[i] = dha[i] + tmp[i];
        __syncthreads();
        } else {
        // Luong: e_j = g (h . keys_j), h the attention cell's new state (A = AS).  dh += g sum_j de_j keys_j, d_keys_j += g de_j h,
        // dg = sum_j de_j (h . keys_j)
        for (int i = tid; i < A; i += kThreads) qb[i] = a.XC[row * (AS + ENC) + i];       // h
        __syncthreads();
        {
            double aq[4] = {0.0, 0.0, 0.0, 0.0}, wdg = 0.0;                          // attention_size <= 256: four columns a lane
            for (int j = wv; j < len; j += kWaves) {
                const float dej = de[j];
                double dot = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = lane + 64 * q;
                    if (i < A) {
                        const float kv = keys[(long long)j * A + i];
                        dot = fma((double)qb[i], (double)kv, dot);
                        aq[q] += (double)(dej * kv);
                        dkeys[(long long)j * A + i] += lg * (dej * qb[i]);
                    }
                }
                wdg += (double)dej * wave_sum(dot);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = lane + 64 * q;
                if (i < A) wp[wv * A + i] = (float)aq[q];
            }
            if (lane == 0) reinterpret_cast<double*>(wp + kWaves * A)[wv] = wdg;
        }
        __syncthreads();
        for (int i = tid; i < A; i += kThreads) {
            double sq = 0.0;
            for (int w = 0; w < kWaves; ++w) sq += (double)wp[w * A + i];
            dhl[i] = dha[i] + lg * (float)sq;
        }
        if (tid == 0) for (int w = 0; w < kWaves; ++w) accsb += reinterpret_cast<double*>(wp + kWaves * A)[w];
        __syncthreads();
        }
        // attention GRU on [prenet_t | context_{t-1}]
        tg_gru_bwd(B + a.w.aWg, B + a.w.aWc, ain, AS, a.XA + row * XW, a.GA + row * 3 * AS, dhl, dx, a.DAg + row * 2 * AS, a.DAc + row * AS,
                   dcl, dgl, dxh, dxh2);
        for (int i = tid; i < D1; i += kThreads) a.DP[row * D1 + i] = dx[i];
        for (int i = tid; i < ENC; i += kThreads) dctx[i] = dx[D1 + i];
        for (int i = tid; i < AS; i += kThreads) dha[i] = dhl[i];
        __syncthreads();
    }
    float* dinit = a.dinit + (long long)n * (AS + L * DR);
    for (int i = tid; i < AS; i += kThreads) dinit[i] = dha[i];
    for (int i = tid; i < L * DR; i += kThreads) dinit[AS + i] = ddech[i];
    for (int i = tid; i < A; i += kThreads) { a.pv[(long long)n * A + i] = (float)accv[i]; a.pb[(long long)n * A + i] = (float)accb[i]; }
    if (tid == 0) a.psb[n] = (float)accsb;
}

// ---- the decoder's own products over rows.  Everything not transposed goes through the shared row kernel (grad_rows_kernel).
constexpr int kRowsK = 512;        // the widest row tg_rows_nt_kernel stages

// Not the CBHG's transpose + row kernel (k in order): here the lanes stride over k and a butterfly adds them, another order of additions.
// C[r][j] (+)= gate_in[r][j] * sum_k X[r][k] W[j][k]  (the product with the transposed kernel; W is (ncols, K) row-major)
__global__ void __launch_bounds__(256) tg_rows_nt_kernel(RowsArgs a)
{
    __shared__ float xs[kRB * kRowsK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r0 = blockIdx.x * kRB, nr = min(kRB, a.rows - r0), K = a.Cin;
    for (int i = tid; i < kRB * K; i += 256) { const int r = i / K, k = i - r * K; xs[i] = r < nr ? a.X[(long long)(r0 + r) * a.ldx + k] : 0.0f; }
    __syncthreads();
    for (int j = wv; j < a.ncols; j += 4) {
        double acc[kRB];
#pragma unroll
        for (int r = 0; r < kRB; ++r) acc[r] = 0.0;
        for (int k = lane; k < K; k += 64) {
            const double w = (double)a.W[(long long)j * a.ldw + k];
#pragma unroll
            for (int r = 0; r < kRB; ++r) acc[r] = fma(w, (double)xs[r * K + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kRB; ++r) {
            const double s = wave_sum(acc[r]);
            if (lane == 0 && r < nr) {
                const long long o = (long long)(r0 + r) * a.ldc + j;
                float v = (float)s;
                if (a.gate_in) v *= a.gate_in[o];
                a.C[o] = a.add ? a.C[o] + v : v;
            }
        }
    }
}

// fed frames of TacoTrainingHelper: F[n][0] = 0 (go frame), F[n][t] = targets[n][t * r - 1]
__global__ void tg_fed_frames_kernel(const float* tgt, int N, int steps, int R, int M, float* F)
{
    const long long total = (long long)N * steps * M;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i % M); const long long row = i / M; const int t = (int)(row % steps); const long long n = row / steps;
        F[i] = t == 0 ? 0.0f : tgt[((n * steps * R) + (long long)t * R - 1) * M + m];
    }
}
// out[j] = sum over rows of D[row][j], rows in order (float64 inside)
// Not the CBHG's cg_colsum_kernel + cg_finish_kernel (chunks of 128 rows, four strided partial sums each): another order of additions.
__global__ void tg_colsum_kernel(const float* D, long long rows, int ld, int ncols, float* out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    double s = 0.0;
    for (long long r = 0; r < rows; ++r) s += (double)D[r * ld + j];
    out[j] = (float)s;
}
// the utterances' partial sums in utterance order; v-hat = g v / ||v||: dv = g / ||v|| (dv-hat - v (v . dv-hat) / ||v||^2), dg = v . dv-hat / ||v||
// AK_SOFT: the same without a score bias.  AK_LUONG: attention_g's gradient alone (psb holds the utterances' dg; `norm` = luong_scaled).
template <int AK>
__global__ void __launch_bounds__(256) tg_attention_finish_kernel(const float* blob, TacoDecoderBlobCore w, int norm, int N, int A, const float* pv,
                                                                  const float* pb, const float* psb, float* grad)
{
    __shared__ double dvh[256];
    const int i = threadIdx.x;
    if constexpr (AK == AK_LUONG) {
        if (i == 0 && norm) {
            double s = 0.0;
            for (int n = 0; n < N; ++n) s += (double)psb[n];
            grad[w.ag] = (float)s;
        }
        return;
    }
    if (i < A) {
        double sv = 0.0, sbb = 0.0;
        for (int n = 0; n < N; ++n) { sv += (double)pv[(long long)n * A + i]; sbb += (double)pb[(long long)n * A + i]; }
        dvh[i] = sv;
        if (norm) grad[w.ab + i] = (float)sbb;
    }
    __syncthreads();
    __shared__ double dot_s, nn_s;
    if (i == 0) {
        double s = 0.0, dot = 0.0, nn = 0.0;
        if constexpr (AK == AK_MON) {
        for (int n = 0; n < N; ++n) s += (double)psb[n];
        grad[w.asb] = (float)s;
        }
        for (int k = 0; k < A; ++k) { const double v = (double)blob[w.av + k]; dot += v * dvh[k]; nn += v * v; }
        dot_s = dot; nn_s = nn;
        if (norm) grad[w.ag] = (float)(dot / sqrt(nn));
    }
    __syncthreads();
    if (i < A) {
        if (norm) {
            const double g = (double)blob[w.ag], nrm = sqrt(nn_s), v = (double)blob[w.av + i];
            grad[w.av + i] = (float)(g / nrm * (dvh[i] - v * dot_s / nn_s));
        } else grad[w.av + i] = (float)dvh[i];
    }
}

// AK_LOC, first half: the utterances' dF (float64) and sum_j g_ja (pb) added in utterance order -> dFs = dF (31 x A), then sg (A);
// attention_variable (not normalised) and attention_bias get their gradients here
__global__ void tg_loc_sum_kernel(TacoDecoderBlob w, int N, int A, const double* pF, const float* pv, const float* pb, double* dFs, float* grad)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < kLocTaps * A) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += pF[(long long)n * kLocTaps * A + idx];
        dFs[idx] = s;
    } else if (idx < (kLocTaps + 1) * A) {
        const int i = idx - kLocTaps * A;
        double sv = 0.0, sg = 0.0;
        for (int n = 0; n < N; ++n) { sv += (double)pv[(long long)n * A + i]; sg += (double)pb[(long long)n * A + i]; }
        dFs[idx] = sg;
        grad[w.av + i] = (float)sv; grad[w.ab + i] = (float)sg;
    }
}
// second half, F = K . L and f_b = conv_b . L + b_a:  dK = dF . L^T,  dL = K^T . dF + conv_b (x) sg,  d conv_b = L . sg
__global__ void tg_loc_finish_kernel(const float* blob, TacoDecoderBlob w, int A, const double* dFs, float* grad)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, nK = kLocTaps * kLocFilters, nL = kLocFilters * A;
    const float *K = blob + w.lcK, *Lk = blob + w.lcL, *cb = blob + w.lcb;
    const double* sg = dFs + kLocTaps * A;
    double s = 0.0;
    if (idx < nK) {
        const int tap = idx / kLocFilters, cc = idx - tap * kLocFilters;
        for (int i = 0; i < A; ++i) s = fma(dFs[tap * A + i], (double)Lk[(long long)cc * A + i], s);
        grad[w.lcK + idx] = (float)s;
    } else if (idx < nK + nL) {
        const int o = idx - nK, cc = o / A, i = o - cc * A;
        for (int tap = 0; tap < kLocTaps; ++tap) s = fma((double)K[tap * kLocFilters + cc], dFs[tap * A + i], s);
        grad[w.lcL + o] = (float)(s + (double)cb[cc] * sg[i]);
    } else if (idx < nK + nL + kLocFilters) {
        const int cc = idx - nK - nL;
        for (int i = 0; i < A; ++i) s = fma((double)Lk[(long long)cc * A + i], sg[i], s);
        grad[w.lcb + cc] = (float)s;
    }
}

__global__ void tg_mel_loss_grad_kernel(const float* mel, const float* tgt, const float* coeff, long long per, float count, long long total, float* out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float d = mel[i] - tgt[i], s = coeff[i / per] / count;
        out[i] = d > 0.0f ? s : (d < 0.0f ? -s : 0.0f);
    }
}

}  // namespace tg
using namespace tg;

static int tg_kind(int attention_type)
{
    switch (attention_type) {
    case TWV_ATT_BAH_MON_NORM: case TWV_ATT_BAH_MON: return AK_MON;
    case TWV_ATT_BAH_NORM: case TWV_ATT_BAH: return AK_SOFT;
    case TWV_ATT_LOC_SEN: return AK_LOC;
    default: return AK_LUONG;
    }
}
// attention_g exists: the normalised Bahdanau scores and luong_scaled
static int tg_has_g(int attention_type)
{
    return attention_type == TWV_ATT_BAH_MON_NORM || attention_type == TWV_ATT_BAH_NORM || attention_type == TWV_ATT_LUONG_SCALED;
}
static const char* tg_attention_name(int attention_type)
{
    static const char* const names[] = {"bah_mon_norm", "bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen"};
    return names[attention_type - TWV_ATT_BAH_MON_NORM];
}

// ---- the workspace of one handle: ONE carve, which also sizes it
struct TgCarve {
    float *F, *H1, *G1, *P, *G2, *keys, *XA, *GA, *XC, *QB, *PCH, *CP, *S, *AL, *XR[4], *GR[4], *YF;
    float *dYF, *DAg, *DAc, *DQ, *DY0, *DRg[4], *DRc[4], *DP, *dH1, *dkeys, *pv, *pb, *psb;
    float *CUM, *LF, *GJ, *U, *pF, *dFs;       // AK_LOC (pF, dFs: float64)
};
struct twv_tacotron_decoder_grad : Handle {
    twv_tacotron_dims d;
    TacoDecoderBlob w;
    int N, T, steps;
    int any = 0;                   // made by _create_any: _reshape validates as it does
    int lds_fwd, lds_bwd;          // bytes
    int forwarded = 0;             // a forward has been made since create
};
using Tg = twv_tacotron_decoder_grad;

static long long tg_carve(const twv_tacotron_decoder_grad* g, float* base, TgCarve& c)
{
    const twv_tacotron_dims& d = g->d;
    const long long rows = (long long)g->N * g->steps, rowsE = (long long)g->N * g->T;
    const int D0 = d.dec_prenet_sizes[0], D1 = d.dec_prenet_sizes[1], ENC = 2 * d.enc_rnn_size, A = d.attention_size, AS = d.attention_state_size,
              DR = d.dec_rnn_size, M = d.num_mels, L = d.dec_layer_num;
    const int ak = tg_kind(d.attention_type);
    TakeFloats take{base};
    c.F = take(rows * M); c.H1 = take(rows * D0); c.G1 = take(rows * D0); c.P = take(rows * D1); c.G2 = take(rows * D1);
    c.keys = take(rowsE * A);
    // the tape by kind: the query layer's output does not exist for Luong, p_choose / cumprod / cumsum are the monotonic kinds' alone
    c.XA = take(rows * (D1 + ENC + 2 * AS)); c.GA = take(rows * 3 * AS); c.XC = take(rows * (AS + ENC));
    c.QB = ak != AK_LUONG ? take(rows * A) : nullptr;
    for (float** p : {&c.PCH, &c.CP, &c.S}) *p = ak == AK_MON ? take(rows * g->T) : nullptr;
    c.AL = take(rows * g->T);
    for (int l = 0; l < 4; ++l) { c.XR[l] = l < L ? take(rows * 3 * DR) : nullptr; c.GR[l] = l < L ? take(rows * 3 * DR) : nullptr; }
    c.YF = take(rows * DR);
    c.dYF = take(rows * DR); c.DAg = take(rows * 2 * AS); c.DAc = take(rows * AS); c.DQ = ak != AK_LUONG ? take(rows * A) : nullptr;
    c.DY0 = take(rows * DR);
    for (int l = 0; l < 4; ++l) { c.DRg[l] = l < L ? take(rows * 2 * DR) : nullptr; c.DRc[l] = l < L ? take(rows * DR) : nullptr; }
    c.DP = take(rows * D1); c.dH1 = take(rows * D0); c.dkeys = take(rowsE * A);
    c.pv = take((long long)g->N * A); c.pb = take((long long)g->N * A); c.psb = take(g->N);
    c.CUM = c.LF = c.GJ = c.U = c.pF = c.dFs = nullptr;
    if (ak == AK_LOC) {
        c.CUM = take(rows * g->T); c.LF = take((kLocTaps + 1) * A); c.GJ = take(rowsE * A); c.U = take(rowsE * 32);
        c.pF = take(2LL * g->N * kLocTaps * A); c.dFs = take(2LL * (kLocTaps + 1) * A);
    }
    return take.off.used;
}

static const char* const kTgBuilt = "the decoder gradient is built for attention_type 'bah_mon_norm' and 'bah_mon', single-speaker and 'deepvoice' models";

// what _create and _reshape accept of (batch, t_in, steps) for the model `d`: one validation, so both answer with the same codes and words.
// Gives the LDS bytes of the two recurrent kernels at t_in.
static int tg_check_sizes(const twv_tacotron_dims& d, int any, int batch, int t_in, int steps, int& lf, int& lb)
{
    if (batch < 1 || t_in < 1 || t_in > 1024) return twv_fail(TWV_E_INVALID, "batch >= 1 and 1 <= t_in <= 1024 required");
    if (steps < 1 || steps > d.max_iters) return twv_fail(TWV_E_INVALID, "steps must satisfy 1 <= steps <= max_iters");
    if (!any && tg_kind(d.attention_type) != AK_MON)
        return twv_fail(TWV_E_UNSUPPORTED, std::string("attention_type: ") + kTgBuilt + " (not bah_norm, bah, luong, luong_scaled, loc_sen)");
    if (d.num_speakers > 1 && d.model_simple && d.speaker_embedding_size != 1)
        return twv_fail(TWV_E_UNSUPPORTED, std::string("model_type 'simple': ") + kTgBuilt);
    const int D0 = d.dec_prenet_sizes[0], D1 = d.dec_prenet_sizes[1], ENC = 2 * d.enc_rnn_size, A = d.attention_size, AS = d.attention_state_size,
              DR = d.dec_rnn_size, L = d.dec_layer_num;
    // twv_tacotron_create has bounded everything else (attention_size, attention_state_size = dec_rnn_size <= 256, dec_prenet_sizes[0] and
    // num_mels * r <= 512, 1 .. 4 layers); the row kernels hold rows of up to 512 floats
    if (D1 > kRowsK || D0 > kRowsK || d.num_mels > kRowsK) return twv_fail(TWV_E_UNSUPPORTED, "decoder gradient: dec_prenet_sizes and num_mels above 512 are not built");
    // Of each carve only the four arrays of Tp = t_in rounded up to 4 floats follow t_in: 16 KB at t_in = 1024.  The rest is bounded by
    // twv_tacotron_create: at its widest (D1 = 512, ENC = 256, A = AS = DR = 256, L = 4) the forward carve is 43 KB and the backward
    // carve 66 KB, so no model it accepts reaches the bound below at t_in <= 1024.  The check stays: it is what holds if a bound moves.
    // (loc_sen adds its combined filter, 31 KB at A = 256, and three more arrays of t_in: 101 KB at the widest)
    const int ak = tg_kind(d.attention_type);
    lf = tg_fwd_lds(t_in, D1, ENC, A, AS, DR, L, ak).total * 4; lb = tg_bwd_lds(t_in, D1, ENC, A, AS, DR, L, ak).total * 4;
    if (lf > 160 * 1024 || lb > 160 * 1024) return twv_fail(TWV_E_UNSUPPORTED, "decoder gradient: the per-utterance state does not fit the LDS of one workgroup");
    return TWV_OK;
}
// everything of a handle that follows (batch, t_in, steps): the sizes, the LDS bytes, the workspace size and the label
static void tg_set_sizes(twv_tacotron_decoder_grad* g, int batch, int t_in, int steps, int lf, int lb)
{
    const twv_tacotron_dims& d = g->d;
    g->N = batch; g->T = t_in; g->steps = steps; g->lds_fwd = lf; g->lds_bwd = lb;
    TgCarve c;
    g->ws_floats = tg_carve(g, nullptr, c);
    g->route = std::string("kernel=tg_bptt attention=") + tg_attention_name(d.attention_type) +
               " workgroups_per_utterance=1 threads=512 layers=" + std::to_string(d.dec_layer_num) + " lds_forward=" + std::to_string(lf) +
               " lds_backward=" + std::to_string(lb) + " wgrad=rocblas";
    g->forwarded = 0;
}

static int tg_create(const twv_tacotron* h, int any, int batch, int t_in, int steps, twv_tacotron_decoder_grad** out)
{
    if (!h || !out) return twv_fail(TWV_E_INVALID, "null argument");
    const twv_tacotron_dims& d = taco_dims(h);
    int lf = 0, lb = 0;
    GRAD_CHK(tg_check_sizes(d, any, batch, t_in, steps, lf, lb));
    twv_tacotron_decoder_grad* g = new twv_tacotron_decoder_grad();
    g->d = d; g->any = any;
    taco_decoder_blob(h, g->w);
    tg_set_sizes(g, batch, t_in, steps, lf, lb);
    *out = g;
    return TWV_OK;
}
// the two monotonic attention types alone, in the words it has always had; _create_any: every attention type twv_tacotron_create accepts
extern "C" int twv_tacotron_decoder_grad_create(const twv_tacotron* h, int batch, int t_in, int steps, twv_tacotron_decoder_grad** out)
{
    return tg_create(h, 0, batch, t_in, steps, out);
}
extern "C" int twv_tacotron_decoder_grad_create_any(const twv_tacotron* h, int batch, int t_in, int steps, twv_tacotron_decoder_grad** out)
{
    return tg_create(h, 1, batch, t_in, steps, out);
}
// The handle at other sizes: what a _create at (batch, t_in, steps) would give, with the rocBLAS handle, the events and the timing flag
// kept (nothing the handle owns depends on the sizes: the tape lives in the caller's workspace, carved anew by every run).  A refused
// call leaves the handle as it was.
extern "C" int twv_tacotron_decoder_grad_reshape(twv_tacotron_decoder_grad* g, int batch, int t_in, int steps)
{
    if (!g) return twv_fail(TWV_E_INVALID, "null argument");
    int lf = 0, lb = 0;
    GRAD_CHK(tg_check_sizes(g->d, g->any, batch, t_in, steps, lf, lb));
    tg_set_sizes(g, batch, t_in, steps, lf, lb);
    return TWV_OK;
}
extern "C" void twv_tacotron_decoder_grad_destroy(twv_tacotron_decoder_grad* g) { delete g; }
extern "C" int twv_tacotron_decoder_grad_set_timing(twv_tacotron_decoder_grad* g, int on) { return g ? g->set_timing(on) : twv_fail(TWV_E_INVALID, "null argument"); }
extern "C" size_t twv_tacotron_decoder_grad_workspace_bytes(const twv_tacotron_decoder_grad* g) { return g ? (size_t)g->ws_floats * 4 : 0; }
extern "C" const char* twv_tacotron_decoder_grad_route(const twv_tacotron_decoder_grad* g) { return g ? g->route.c_str() : ""; }

// C (rows x ncols) = X (rows x K) . W (K x ncols) + bias through the shared row kernel, every matrix dense; the caller adds the relu's
// mask and gate to the arguments
static RowsArgs tg_nn(const float* X, int rows, int K, const float* W, int ncols, const float* bias, float* C)
{
    RowsArgs a = rows_args(X, K, rows, rows, K, 1, 0, W, ncols, ncols, bias);
    a.C = C; a.ldc = ncols;
    return a;
}
// C (rows x ncols) = X (rows x K) . W^T, W (ncols x K); the caller sets gate_in / add
static RowsArgs tg_nt(const float* X, int rows, int K, const float* W, int ncols, float* C)
{
    RowsArgs a = rows_args(X, K, rows, rows, K, 1, 0, W, K, ncols, nullptr);
    a.C = C; a.ldc = ncols;
    return a;
}
static void tg_launch_nt(hipStream_t st, const RowsArgs& a) { hipLaunchKernelGGL(tg_rows_nt_kernel, dim3((a.rows + kRB - 1) / kRB), dim3(256), 0, st, a); }

namespace {
// the arguments of the two recurrent kernels: the tape and the deltas are pieces of the workspace (AK_LOC: with its own behind them)
TgLocArgs tg_args(const Tg* g, const float* blob, const float* memory, const float* decoder_init, const int32_t* lengths, const TgCarve& c, float* d_memory,
               float* d_init)
{
    const twv_tacotron_dims& d = g->d;
    TgLocArgs a;
    memset(&a, 0, sizeof(a));
    a.blob = blob; a.memory = memory; a.init = decoder_init; a.keys = c.keys; a.lengths = lengths; a.w = g->w;
    a.N = g->N; a.T = g->T; a.steps = g->steps; a.D1 = d.dec_prenet_sizes[1]; a.ENC = 2 * d.enc_rnn_size; a.A = d.attention_size; a.AS = d.attention_state_size;
    a.DR = d.dec_rnn_size; a.L = d.dec_layer_num; a.norm = tg_has_g(d.attention_type);
    a.P = c.P; a.XA = c.XA; a.GA = c.GA; a.XC = c.XC; a.QB = c.QB; a.PCH = c.PCH; a.CP = c.CP; a.S = c.S; a.AL = c.AL; a.YF = c.YF;
    for (int l = 0; l < 4; ++l) { a.XR[l] = c.XR[l]; a.GR[l] = c.GR[l]; a.DRg[l] = c.DRg[l]; a.DRc[l] = c.DRc[l]; }
    a.dYF = c.dYF; a.DAg = c.DAg; a.DAc = c.DAc; a.DQ = c.DQ; a.DY0 = c.DY0; a.DP = c.DP; a.dkeys = c.dkeys; a.dmem = d_memory; a.dinit = d_init;
    a.pv = c.pv; a.pb = c.pb; a.psb = c.psb;
    a.CUM = c.CUM; a.F = c.LF; a.GJ = c.GJ; a.U = c.U; a.pF = reinterpret_cast<double*>(c.pF);
    return a;
}
// one workgroup an utterance on the instantiation of the model's kind; the kinds but AK_LOC receive the TgArgs part of the arguments
template <int AK>
int tg_launch(void (*kernel)(typename TgArgsOf<AK>::type), int N, int lds_bytes, hipStream_t st, const TgLocArgs& a)
{
    GRAD_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    const typename TgArgsOf<AK>::type ka = a;
    hipLaunchKernelGGL(kernel, dim3(N), dim3(kThreads), (size_t)lds_bytes, st, ka);
    return TWV_OK;
}
}  // namespace

// ---- the two halves of a pass: the tape of a forward stays in the caller's workspace until the handle's next forward
extern "C" int twv_tacotron_decoder_grad_forward(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                                 const int32_t* lengths, const float* mel_targets, const float* mask1, const float* mask2,
                                                 void* workspace, int32_t* status, void* stream, float* mel_out)
{
    if (!g || !blob || !memory || !decoder_init || !lengths || !mel_targets || !workspace || !status || !mel_out) return twv_fail(TWV_E_INVALID, "null argument");
    const twv_tacotron_dims& d = g->d;
    const TacoDecoderBlob& w = g->w;
    hipStream_t st = (hipStream_t)stream;
    const int N = g->N, T = g->T, steps = g->steps, rows = N * steps, rowsE = N * T;
    const int D0 = d.dec_prenet_sizes[0], D1 = d.dec_prenet_sizes[1], ENC = 2 * d.enc_rnn_size, A = d.attention_size, DR = d.dec_rnn_size, M = d.num_mels,
              R = d.reduction_factor, MR = M * R;
    GRAD_CHK(g->begin(st, status, nullptr, w.blob_floats));
    TgCarve c;
    tg_carve(g, (float*)workspace, c);
    // ---- (a) recording forward
    GRAD_CHK(g->mark(0));
    hipLaunchKernelGGL(tg_fed_frames_kernel, dim3(grid_for((long long)rows * M)), dim3(256), 0, st, mel_targets, N, steps, R, M, c.F);
    {
        RowsArgs p = tg_nn(c.F, rows, M, blob + w.dpW1, D0, blob + w.dpb1, c.H1);
        p.act = 1; p.mask = mask1; p.gate_out = c.G1;
        launch_rows<Tg>(st, p);
        p = tg_nn(c.H1, rows, D0, blob + w.dpW2, D1, blob + w.dpb2, c.P);
        p.act = 1; p.mask = mask2; p.gate_out = c.G2;
        launch_rows<Tg>(st, p);
        launch_rows<Tg>(st, tg_nn(memory, rowsE, ENC, blob + w.Wm, A, nullptr, c.keys));
    }
    const TgLocArgs a = tg_args(g, blob, memory, decoder_init, lengths, c, nullptr, nullptr);
    const int ak = tg_kind(d.attention_type);
    if (ak == AK_LOC)
        hipLaunchKernelGGL(tg_loc_derive_kernel, dim3(((kLocTaps + 1) * A + 255) / 256), dim3(256), 0, st, blob, w, A, c.LF);
    GRAD_CHK(ak == AK_MON ? tg_launch<AK_MON>(tg_forward_kernel<AK_MON>, N, g->lds_fwd, st, a)
             : ak == AK_SOFT ? tg_launch<AK_SOFT>(tg_forward_kernel<AK_SOFT>, N, g->lds_fwd, st, a)
             : ak == AK_LUONG ? tg_launch<AK_LUONG>(tg_forward_kernel<AK_LUONG>, N, g->lds_fwd, st, a)
             : tg_launch<AK_LOC>(tg_forward_kernel<AK_LOC>, N, g->lds_fwd, st, a));
    launch_rows<Tg>(st, tg_nn(c.YF, rows, DR, blob + w.oW, MR, blob + w.ob, mel_out));
    GRAD_HIPCHK(hipGetLastError());
    g->forwarded = 1;
    return TWV_OK;
}

extern "C" int twv_tacotron_decoder_grad_backward(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                                  const int32_t* lengths, const float* d_mel, void* workspace, int32_t* status, void* stream,
                                                  float* grad_blob, float* d_memory, float* d_init)
{
    if (!g || !blob || !memory || !decoder_init || !lengths || !d_mel || !workspace || !status || !grad_blob || !d_memory || !d_init)
        return twv_fail(TWV_E_INVALID, "null argument");
    if (!g->forwarded) return twv_fail(TWV_E_INVALID, "backward: no forward has been made on this handle (twv_tacotron_decoder_grad_forward)");
    const twv_tacotron_dims& d = g->d;
    const TacoDecoderBlob& w = g->w;
    hipStream_t st = (hipStream_t)stream;
    const int N = g->N, T = g->T, steps = g->steps, rows = N * steps, rowsE = N * T;
    const int D0 = d.dec_prenet_sizes[0], D1 = d.dec_prenet_sizes[1], ENC = 2 * d.enc_rnn_size, A = d.attention_size, AS = d.attention_state_size,
              DR = d.dec_rnn_size, M = d.num_mels, R = d.reduction_factor, L = d.dec_layer_num, MR = M * R, ain = D1 + ENC, XW = ain + 2 * AS;
    const int norm = tg_has_g(d.attention_type), ak = tg_kind(d.attention_type);
    GRAD_CHK(g->begin(st, status, grad_blob, w.blob_floats));
    TgCarve c;
    tg_carve(g, (float*)workspace, c);
    const TgLocArgs a = tg_args(g, blob, memory, decoder_init, lengths, c, d_memory, d_init);
    // ---- (b) backward through time
    GRAD_CHK(g->mark(1));
    tg_launch_nt(st, tg_nt(d_mel, rows, MR, blob + w.oW, DR, c.dYF));
    GRAD_CHK(ak == AK_MON ? tg_launch<AK_MON>(tg_backward_kernel<AK_MON>, N, g->lds_bwd, st, a)
             : ak == AK_SOFT ? tg_launch<AK_SOFT>(tg_backward_kernel<AK_SOFT>, N, g->lds_bwd, st, a)
             : ak == AK_LUONG ? tg_launch<AK_LUONG>(tg_backward_kernel<AK_LUONG>, N, g->lds_bwd, st, a)
             : tg_launch<AK_LOC>(tg_backward_kernel<AK_LOC>, N, g->lds_bwd, st, a));
    {
        RowsArgs p = tg_nt(c.dkeys, rowsE, A, blob + w.Wm, ENC, d_memory);
        p.add = 1;                                                                   // d_values += d_keys . Wm^T
        tg_launch_nt(st, p);
        launch_mul<Tg>(st, c.DP, c.G2, (long long)rows * D1);
        p = tg_nt(c.DP, rows, D1, blob + w.dpW2, D0, c.dH1);
        p.gate_in = c.G1;
        tg_launch_nt(st, p);
    }
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(g->mark(2));
    // ---- (c) weight gradients: grad[K x N] = X^T (K x rows) . delta (rows x N), row-major = rocBLAS (N x K) = delta^T-as-stored . X
    auto colsum = [&](const float* D, int ld, int Nc, long long off, long long nrows) {
        hipLaunchKernelGGL(tg_colsum_kernel, dim3((Nc + 63) / 64), dim3(64), 0, st, D, nrows, ld, Nc, grad_blob + off);
    };
    GRAD_CHK(g->wgrad(c.YF, DR, DR, d_mel, MR, MR, w.oW, rows)); colsum(d_mel, MR, MR, w.ob, rows);
    for (int l = 0; l < L; ++l) {
        GRAD_CHK(g->wgrad(c.XR[l], 3 * DR, 2 * DR, c.DRg[l], 2 * DR, 2 * DR, w.rWg[l], rows)); colsum(c.DRg[l], 2 * DR, 2 * DR, w.rbg[l], rows);
        GRAD_CHK(g->wgrad(c.XR[l], 3 * DR, DR, c.DRc[l], DR, DR, w.rWc[l], rows));
        GRAD_CHK(g->wgrad(c.XR[l] + 2 * DR, 3 * DR, DR, c.DRc[l], DR, DR, w.rWc[l] + (long long)DR * DR, rows));
        colsum(c.DRc[l], DR, DR, w.rbc[l], rows);
    }
    GRAD_CHK(g->wgrad(c.XC, AS + ENC, AS + ENC, c.DY0, DR, DR, w.cW, rows)); colsum(c.DY0, DR, DR, w.cb, rows);
    if (ak != AK_LUONG) GRAD_CHK(g->wgrad(c.XC, AS + ENC, AS, c.DQ, A, A, w.Wq, rows));
    GRAD_CHK(g->wgrad(c.XA, XW, ain + AS, c.DAg, 2 * AS, 2 * AS, w.aWg, rows)); colsum(c.DAg, 2 * AS, 2 * AS, w.abg, rows);
    GRAD_CHK(g->wgrad(c.XA, XW, ain, c.DAc, AS, AS, w.aWc, rows));
    GRAD_CHK(g->wgrad(c.XA + ain + AS, XW, AS, c.DAc, AS, AS, w.aWc + (long long)ain * AS, rows));
    colsum(c.DAc, AS, AS, w.abc, rows);
    GRAD_CHK(g->wgrad(c.H1, D0, D0, c.DP, D1, D1, w.dpW2, rows)); colsum(c.DP, D1, D1, w.dpb2, rows);
    GRAD_CHK(g->wgrad(c.F, M, M, c.dH1, D0, D0, w.dpW1, rows)); colsum(c.dH1, D0, D0, w.dpb1, rows);
    GRAD_CHK(g->wgrad(memory, ENC, ENC, c.dkeys, A, A, w.Wm, rowsE));
    if (ak == AK_MON) hipLaunchKernelGGL(tg_attention_finish_kernel<AK_MON>, dim3(1), dim3(256), 0, st, blob, w, norm, N, A, c.pv, c.pb, c.psb, grad_blob);
    else if (ak == AK_SOFT) hipLaunchKernelGGL(tg_attention_finish_kernel<AK_SOFT>, dim3(1), dim3(256), 0, st, blob, w, norm, N, A, c.pv, c.pb, c.psb, grad_blob);
    else if (ak == AK_LUONG) hipLaunchKernelGGL(tg_attention_finish_kernel<AK_LUONG>, dim3(1), dim3(256), 0, st, blob, w, norm, N, A, c.pv, c.pb, c.psb, grad_blob);
    else {
        double* dFs = reinterpret_cast<double*>(c.dFs);
        hipLaunchKernelGGL(tg_loc_sum_kernel, dim3(((kLocTaps + 1) * A + 255) / 256), dim3(256), 0, st, w, N, A, reinterpret_cast<const double*>(c.pF),
                           c.pv, c.pb, dFs, grad_blob);
        hipLaunchKernelGGL(tg_loc_finish_kernel, dim3((kLocTaps * kLocFilters + kLocFilters * A + kLocFilters + 255) / 256), dim3(256), 0, st, blob, w,
                           A, dFs, grad_blob);
    }
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(g->mark(3));
    return TWV_OK;
}

// forward, then backward
extern "C" int twv_tacotron_decoder_grad_run(twv_tacotron_decoder_grad* g, const float* blob, const float* memory, const float* decoder_init,
                                             const int32_t* lengths, const float* mel_targets, const float* d_mel, const float* mask1,
                                             const float* mask2, void* workspace, int32_t* status, void* stream, float* mel_out,
                                             float* grad_blob, float* d_memory, float* d_init)
{
    if (!g || !blob || !memory || !decoder_init || !lengths || !mel_targets || !d_mel || !workspace || !status || !mel_out || !grad_blob ||
        !d_memory || !d_init)
        return twv_fail(TWV_E_INVALID, "null argument");
    GRAD_CHK(twv_tacotron_decoder_grad_forward(g, blob, memory, decoder_init, lengths, mel_targets, mask1, mask2, workspace, status, stream, mel_out));
    return twv_tacotron_decoder_grad_backward(g, blob, memory, decoder_init, lengths, d_mel, workspace, status, stream, grad_blob, d_memory, d_init);
}

// after a run with timing on: waits for it and gives the milliseconds of (a) the recording forward, (b) the backward through time (with the
// prenet backward and d_memory's memory_layer term) and (c) the weight-gradient products
extern "C" int twv_tacotron_decoder_grad_phase_ms(twv_tacotron_decoder_grad* g, double* ms3)
{
    if (!g || !ms3) return twv_fail(TWV_E_INVALID, "null argument");
    return g->phase_ms(3, ms3, "twv_tacotron_decoder_grad_set_timing");
}

extern "C" int twv_tacotron_mel_loss_grad(const float* mel, const float* mel_targets, const float* loss_coeff, int batch, int t_out,
                                          int num_mels, float* d_mel, void* stream)
{
    if (!mel || !mel_targets || !loss_coeff || !d_mel) return twv_fail(TWV_E_INVALID, "null argument");
    if (batch < 1 || t_out < 1 || num_mels < 1) return twv_fail(TWV_E_INVALID, "batch, t_out and num_mels must be >= 1");
    const long long per = (long long)t_out * num_mels, total = per * batch;
    hipLaunchKernelGGL(tg_mel_loss_grad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, mel, mel_targets, loss_coeff, per,
                       (float)total, total, d_mel);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}
