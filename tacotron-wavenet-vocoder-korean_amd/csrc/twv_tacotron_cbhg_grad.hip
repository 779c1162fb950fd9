// Tacotron encoder and post-net gradients (gfx950): the vector-Jacobian product of one CBHG (modules.py:25-74), instantiated twice
// (DESIGN 3b-h).
//
//   encoder:  d_memory  ->  the gradient of embedding, prenet/* and encoder_cbhg/*  + d_before_highway + d_rnn_init
//   post net: d_linear  ->  the gradient of post_cbhg/* and the linear-spectrogram layer + d_mel (the cotangent on the post net's input)
//
// The pass is (a) a recording forward -- every product over all N * T rows, then cg_gru_forward_kernel, ONE workgroup of 512 threads per
// (utterance, direction), whose recurrent weights (the h rows of gates/kernel and candidate/kernel, 49 152 floats) stay in registers for
// the whole launch; the input halves x . W_x of both GRU kernels are products over all rows made before the loop; (b) cg_gru_backward_kernel,
// the same geometry with the same 49 152 values in the layout of the transposed products, walking each direction's steps backwards with
// dh in LDS and writing the pre-activation deltas per row; (c) the row-wise backward: dx = delta . W_x^T as products over all rows, the
// highway layers, the projections' and the conv bank's batch norm / relu / max-pool backward as fused pointwise kernels with per-channel
// partial sums; (d) every kernel gradient as a product X^T . delta (rocBLAS, atomics off; a convolution as one product per tap against a
// delta whose rows that would read across an utterance boundary are zeroed) and every bias gradient as a column sum.
// No workgroup waits for another one: no exchange areas, tickets or grid barriers.  No atomics: two runs give the same bits.  Whatever lies
// on the path to d_x / d_before_highway / d_rnn_init / the recorded output goes through this file's own row kernel, whose order of additions
// for a row does not depend on how many rows there are: an utterance's outputs are the same bits alone and inside a batch.
#include "twv_tacotron_blob.hpp"
#include "twv_tacotron_grad_common.hpp"

namespace cg {

using namespace tgrad;

constexpr int kU = 128;                              // GRU / highway width: twv_tacotron_create accepts no other enc_rnn_size / post_rnn_size
constexpr int kGruThreads = 512;
constexpr int kChunk = 128;                          // rows per block of the column-statistics kernels

// a workgroup barrier that orders LDS only: __syncthreads() also waits for every global load and store in flight (vmcnt(0)), which in the
// recurrent kernels are the tape writes and the next step's prefetch
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the kernel of the transposed convolution: Wt[(tap' * ncols + j) * Cin + k] = W[((kw - 1 - tap') * Cin + k) * ldw + j]
__global__ void cg_transpose_kernel(const float* W, int kw, int Cin, int ncols, int ldw, float* Wt)
{
    const long long total = (long long)kw * Cin * ncols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Cin); const long long q = i / Cin; const int j = (int)(q % ncols), tp = (int)(q / ncols);
        Wt[i] = W[((long long)(kw - 1 - tp) * Cin + k) * ldw + j];
    }
}

// ---- small row-wise kernels
// tacotron.py:51-60: the <PAD> row of the table reads as zeros
__global__ void cg_embed_kernel(const float* table, const int32_t* tokens, int rows, int E, int nsym, float* out)
{
    const long long total = (long long)rows * E;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(i / E), c = (int)(i - (long long)row * E), tok = tokens[row];
        out[i] = (tok <= 0 || tok >= nsym) ? 0.0f : table[(long long)tok * E + c];
    }
}
// d embedding: a segmented sum, one workgroup per symbol walking the token rows in order (float64 inside); row 0 is exactly zero, as the
// forward never reads it
__global__ void __launch_bounds__(256) cg_embed_grad_kernel(const float* dE, const int32_t* tokens, int rows, int E, float* out)
{
    const int s = blockIdx.x;
    for (int c = threadIdx.x; c < E; c += 256) {
        double acc = 0.0;
        if (s > 0) for (int r = 0; r < rows; ++r) if (tokens[r] == s) acc += (double)dE[(long long)r * E + c];
        out[(long long)s * E + c] = (float)acc;
    }
}
// per-group vectors of the conv bank (one batch norm per convolution): channel c belongs to group c / gs
struct Groups { long long inv[17], shift[17]; int gs; };
// modules.py:38 max_pooling1d(2, stride 1, 'same') on BN(a): out[t] = max(y[t], y[t+1]) inside each utterance
__global__ void cg_pool_kernel(const float* A, const float* blob, Groups g, int rows, int T, int Cn, float* out)
{
    const long long total = (long long)rows * Cn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(i / Cn), c = (int)(i - (long long)row * Cn), q = c / g.gs, cc = c - q * g.gs;
        const float inv = blob[g.inv[q] + cc], sh = blob[g.shift[q] + cc];
        const float y = A[i] * inv + sh;
        float m = y;
        if (row % T + 1 < T) { const float yn = A[i + Cn] * inv + sh; m = yn > y ? yn : y; }
        out[i] = m;
    }
}
// batch norm (inference form y = a * inv + shift) and relu backward, with the max pool in front of it when pool is set:
//   pool: dy[t] = dP[t] where y[t+1] does not beat y[t] (a tie goes to the earlier position)  +  dP[t-1] where y[t] beats y[t-1]
//   dz = dy * inv, 0 where relu and a <= 0;  partial sums over the block's rows of d_inv = dy * a and d_shift = dy (float64)
// grid (column blocks of 64, row chunks of kChunk); a thread walks every fourth row of its column, the four are added in order.
__global__ void __launch_bounds__(256) cg_bn_bwd_kernel(const float* dY, int ldy, const float* A, int lda, const float* blob, Groups g, int rows, int T,
                                                        int Cn, int pool, int relu, float* dZ, int ldz, double* partial)
{
    __shared__ double red[2][4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q4 = threadIdx.x >> 6, ra = blockIdx.y * kChunk, rb = min(rows, ra + kChunk);
    double si = 0.0, ss = 0.0;
    if (c < Cn) {
        const int q = c / g.gs, cc = c - q * g.gs;
        const float inv = blob[g.inv[q] + cc], sh = blob[g.shift[q] + cc];
        for (int r = ra + q4; r < rb; r += 4) {
            const float av = A[(long long)r * lda + c];
            float dy;
            if (pool) {
                const int t = r % T;
                const float y = av * inv + sh;
                dy = 0.0f;
                bool mine = true;
                if (t + 1 < T) { const float yn = A[(long long)(r + 1) * lda + c] * inv + sh; mine = !(yn > y); }
                if (mine) dy += dY[(long long)r * ldy + c];
                if (t > 0) { const float yp = A[(long long)(r - 1) * lda + c] * inv + sh; if (y > yp) dy += dY[(long long)(r - 1) * ldy + c]; }
            } else dy = dY[(long long)r * ldy + c];
            float dz = dy * inv;
            if (relu && !(av > 0.0f)) dz = 0.0f;
            dZ[(long long)r * ldz + c] = dz;
            si += (double)dy * (double)av; ss += (double)dy;
        }
    }
    red[0][q4][threadIdx.x & 63] = si; red[1][q4][threadIdx.x & 63] = ss;
    __syncthreads();
    if (q4 == 0 && c < Cn) {
        const int l = threadIdx.x;
        partial[((long long)blockIdx.y * 2 + 0) * Cn + c] = ((red[0][0][l] + red[0][1][l]) + red[0][2][l]) + red[0][3][l];
        partial[((long long)blockIdx.y * 2 + 1) * Cn + c] = ((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l];
    }
}
// column sums (bias gradients), the same grid: partial[chunk][0][c]
__global__ void __launch_bounds__(256) cg_colsum_kernel(const float* D, int ld, int rows, int Cn, double* partial)
{
    __shared__ double red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q4 = threadIdx.x >> 6, ra = blockIdx.y * kChunk, rb = min(rows, ra + kChunk);
    double s = 0.0;
    if (c < Cn) for (int r = ra + q4; r < rb; r += 4) s += (double)D[(long long)r * ld + c];
    red[q4][threadIdx.x & 63] = s;
    __syncthreads();
    if (q4 == 0 && c < Cn) { const int l = threadIdx.x; partial[(long long)blockIdx.y * Cn + c] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]; }
}
// the chunks' partial sums in chunk order: stat s of channel c goes to grad[off[s][c / gs] + c % gs]
struct FinishArgs { long long off[2][17]; int gs, nstat, Cn, nchunk; };
__global__ void cg_finish_kernel(const double* partial, FinishArgs f, float* grad)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= f.Cn) return;
    const int q = c / f.gs, cc = c - q * f.gs;
    for (int s = 0; s < f.nstat; ++s) {
        double v = 0.0;
        for (int k = 0; k < f.nchunk; ++k) v += partial[((long long)k * f.nstat + s) * f.Cn + c];
        grad[f.off[s][q] + cc] = (float)v;
    }
}
// ---- batch-statistics batch norm (tf.layers.batch_normalization(training=True)).  A handle in batch mode keeps, per batch
// norm and in the order bank 1 .. K, proj_1, proj_2, a (2, C) piece of two buffers of its own: `stats` = (mean, variance) of the last
// forward over ALL rows, `pairs` = the (inv, shift) pair derived from them.  Batch norm q of a launch has its pieces at pair[q] of both
// buffers and its (4, C) tensor (gamma, beta first) at var[q] of the training vector.
const float kCgBnEps = 1e-3f;        // tf.layers.batch_normalization's default epsilon
struct BatchGroups { long long pair[17], var[17]; int gs; };
// column sums of a and a * a (float64), the grid of cg_bn_bwd_kernel: partial[chunk][0 | 1][c]
__global__ void __launch_bounds__(256) cg_stats_kernel(const float* A, int lda, int rows, int Cn, double* partial)
{
    __shared__ double red[2][4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q4 = threadIdx.x >> 6, ra = blockIdx.y * kChunk, rb = min(rows, ra + kChunk);
    double s1 = 0.0, s2 = 0.0;
    if (c < Cn) for (int r = ra + q4; r < rb; r += 4) { const double av = (double)A[(long long)r * lda + c]; s1 += av; s2 += av * av; }
    red[0][q4][threadIdx.x & 63] = s1; red[1][q4][threadIdx.x & 63] = s2;
    __syncthreads();
    if (q4 == 0 && c < Cn) {
        const int l = threadIdx.x;
        partial[((long long)blockIdx.y * 2 + 0) * Cn + c] = ((red[0][0][l] + red[0][1][l]) + red[0][2][l]) + red[0][3][l];
        partial[((long long)blockIdx.y * 2 + 1) * Cn + c] = ((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l];
    }
}
// the chunks in order: mean = sum a / R, variance = sum a^2 / R - mean^2 (biased, float64, clamped at 0), each rounded once to float32; then
// the pair from the float32 statistics in the rounding sequence of tt_refold_kernel / tacotron.bn_inference_vectors
__global__ void cg_stats_finish_kernel(const double* partial, BatchGroups b, int Cn, int nchunk, int rows, const float* variables, float* stats,
                                       float* pairs)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Cn) return;
    const int q = c / b.gs, cc = c - q * b.gs;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nchunk; ++k) { s1 += partial[((long long)k * 2 + 0) * Cn + c]; s2 += partial[((long long)k * 2 + 1) * Cn + c]; }
    const double mu = s1 / (double)rows;
    double v = s2 / (double)rows - mu * mu;
    if (!(v > 0.0)) v = 0.0;
    const float mean = (float)mu, variance = (float)v;
    const float gamma = variables[b.var[q] + cc], beta = variables[b.var[q] + b.gs + cc];
    const float root = (float)sqrt((double)__fadd_rn(variance, kCgBnEps));
    const float inv = __fmul_rn((float)(1.0 / (double)root), gamma);
    stats[b.pair[q] + cc] = mean; stats[b.pair[q] + b.gs + cc] = variance;
    pairs[b.pair[q] + cc] = inv; pairs[b.pair[q] + b.gs + cc] = __fsub_rn(beta, __fmul_rn(mean, inv));
}
// Y = A * inv + shift (+ add1[r] + add2[r / T]): what the row kernel fuses into a projection in inference mode, the same expression in the
// same order (the statistics need all of A first)
__global__ void cg_bn_apply_kernel(const float* A, const float* inv, const float* shift, const float* add1, int ld1, const float* add2, int ld2,
                                   int rows, int T, int Cn, float* Y)
{
    const long long total = (long long)rows * Cn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / Cn; const int j = (int)(i - row * Cn);
        const float v = A[i];
        float y = v * inv[j] + shift[j];
        if (add1) y = y + add1[row * ld1 + j];
        if (add2) y = y + add2[(row / T) * ld2 + j];
        Y[i] = y;
    }
}
// backward, the sums phase: cg_bn_bwd_kernel's routing through the max pool (on the batch pair) and its partial sums of dy * a and dy, but
// dZ receives dy itself -- the elementwise phase needs the finished sums
__global__ void __launch_bounds__(256) cg_bn_batch_sums_kernel(const float* dY, int ldy, const float* A, int lda, const float* pairs, Groups g, int rows,
                                                               int T, int Cn, int pool, float* dZ, int ldz, double* partial)
{
    __shared__ double red[2][4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q4 = threadIdx.x >> 6, ra = blockIdx.y * kChunk, rb = min(rows, ra + kChunk);
    double si = 0.0, ss = 0.0;
    if (c < Cn) {
        const int q = c / g.gs, cc = c - q * g.gs;
        const float inv = pairs[g.inv[q] + cc], sh = pairs[g.shift[q] + cc];
        for (int r = ra + q4; r < rb; r += 4) {
            const float av = A[(long long)r * lda + c];
            float dy;
            if (pool) {
                const int t = r % T;
                const float y = av * inv + sh;
                dy = 0.0f;
                bool mine = true;
                if (t + 1 < T) { const float yn = A[(long long)(r + 1) * lda + c] * inv + sh; mine = !(yn > y); }
                if (mine) dy += dY[(long long)r * ldy + c];
                if (t > 0) { const float yp = A[(long long)(r - 1) * lda + c] * inv + sh; if (y > yp) dy += dY[(long long)(r - 1) * ldy + c]; }
            } else dy = dY[(long long)r * ldy + c];
            dZ[(long long)r * ldz + c] = dy;
            si += (double)dy * (double)av; ss += (double)dy;
        }
    }
    red[0][q4][threadIdx.x & 63] = si; red[1][q4][threadIdx.x & 63] = ss;
    __syncthreads();
    if (q4 == 0 && c < Cn) {
        const int l = threadIdx.x;
        partial[((long long)blockIdx.y * 2 + 0) * Cn + c] = ((red[0][0][l] + red[0][1][l]) + red[0][2][l]) + red[0][3][l];
        partial[((long long)blockIdx.y * 2 + 1) * Cn + c] = ((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l];
    }
}
// the chunks in order: S1 = sum dy, S2 = sum dy * a.  With rs = rsqrt(var + eps): sum dy * xhat = rs (S2 - mean S1), so
// d_gamma = rs (S2 - mean S1) and d_beta = S1 go to the pair's slots of the gradient (gr), and the elementwise phase gets
// coef[0][c] = S1 / R, coef[1][c] = rs^2 (S2 - mean S1) / R
__global__ void cg_bn_batch_finish_kernel(const double* partial, BatchGroups b, Groups gr, int Cn, int nchunk, int rows, const float* stats, double* coef,
                                          float* grad)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Cn) return;
    const int q = c / b.gs, cc = c - q * b.gs;
    double s2 = 0.0, s1 = 0.0;
    for (int k = 0; k < nchunk; ++k) { s2 += partial[((long long)k * 2 + 0) * Cn + c]; s1 += partial[((long long)k * 2 + 1) * Cn + c]; }
    const double mu = (double)stats[b.pair[q] + cc], rs = 1.0 / sqrt((double)stats[b.pair[q] + b.gs + cc] + (double)kCgBnEps);
    const double t = s2 - mu * s1;
    grad[gr.inv[q] + cc] = (float)(rs * t);
    grad[gr.shift[q] + cc] = (float)s1;
    coef[c] = s1 / (double)rows;
    coef[Cn + c] = rs * rs * t / (double)rows;
}
// the elementwise phase, in place on dZ = dy: da = inv (dy - S1 / R - (a - mean) rs^2 (S2 - mean S1) / R), 0 where relu and a <= 0
__global__ void cg_bn_batch_bwd_kernel(float* dZ, int ldz, const float* A, int lda, const float* pairs, const float* stats, BatchGroups b,
                                       const double* coef, int rows, int Cn, int relu)
{
    const long long total = (long long)rows * Cn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / Cn; const int c = (int)(i - r * Cn), q = c / b.gs, cc = c - q * b.gs;
        const float av = A[r * lda + c];
        const double d = ((double)dZ[r * ldz + c] - coef[c]) - ((double)av - (double)stats[b.pair[q] + cc]) * coef[Cn + c];
        float dz = (float)((double)pairs[b.pair[q] + cc] * d);
        if (relu && !(av > 0.0f)) dz = 0.0f;
        dZ[r * ldz + c] = dz;
    }
}
// highway layer: y = relu(h) * sigmoid(t) + x * (1 - sigmoid(t));  H, Tg hold relu(h) and sigmoid(t)
__global__ void cg_highway_kernel(const float* x, const float* H, const float* Tg, long long total, float* y)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        y[i] = H[i] * Tg[i] + x[i] * (1.0f - Tg[i]);
}
// its backward in one pass: D[r] = [dh~ | dt~] (pre-activation deltas, 2 * kU a row), dx = the carry term dy * (1 - sigmoid(t))
__global__ void cg_highway_bwd_kernel(const float* dy, const float* x, const float* H, const float* Tg, long long total, float* D, float* dx)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / kU; const int j = (int)(i - r * kU);
        const float d = dy[i], h = H[i], t = Tg[i];
        D[r * 2 * kU + j] = h > 0.0f ? d * t : 0.0f;
        D[r * 2 * kU + kU + j] = d * (h - x[i]) * t * (1.0f - t);
        dx[i] = d * (1.0f - t);
    }
}
// out[n][j] = sum_t D[n * T + t][j], t in order (float64 inside): d_before_highway
__global__ void cg_utterance_sum_kernel(const float* D, int N, int T, int Cn, float* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * Cn) return;
    const int n = i / Cn, j = i - n * Cn;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)D[((long long)n * T + t) * Cn + j];
    out[i] = (float)s;
}
// Ds[r][j] = D[r][j] where row r + shift lies in r's utterance, else 0: the delta of one tap of a convolution's kernel gradient
__global__ void cg_shift_mask_kernel(const float* D, int ld, int rows, int T, int Cn, int shift, float* Ds)
{
    const long long total = (long long)rows * Cn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / Cn), j = (int)(i - (long long)r * Cn), t = r % T + shift;
        Ds[i] = (t >= 0 && t < T) ? D[(long long)r * ld + j] : 0.0f;
    }
}
__global__ void cg_linear_loss_grad_kernel(const float* lin, const float* tgt, const float* coeff, long long per, int F, int lo, int hi, float w0,
                                           float w1, long long total, float* out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i % F);
        const float d = lin[i] - tgt[i], s = coeff[i / per] * ((f >= lo && f < hi) ? w0 + w1 : w0);
        out[i] = d > 0.0f ? s : (d < 0.0f ? -s : 0.0f);
    }
}

// ---- the bidirectional GRU: blockIdx.x = 2 * utterance + direction, 512 threads
struct GruArgs {
    const float *Wg[2], *Wc[2];          // gates/kernel (2 kU x 2 kU), candidate/kernel (2 kU x kU), rows [x | h]
    const float *GX, *CX;                // x . W_x + bias of all rows: [row][dir][2 kU], [row][dir][kU]
    const float* init;                   // (N, 2 kU) = [fw | bw] or null
    const int32_t* lengths;              // null: every row is live (the post net)
    float* out;                          // (rows, 2 kU), zero past each length
    float *HP[2], *RU[2], *CC[2], *RH[2];   // tape per direction: h_{t-1}, [r | u], c, r * h_{t-1}
    const float* dOut;
    float *DG[2], *DC[2], *dinit;        // [dr~ | du~], dc~ per row (zero past each length); d_rnn_init (N, 2 kU) or null
    int N, T;
};
// LDS of the two recurrent kernels, in floats: one carve for the kernels and for the launch
struct GruLds { int h, g, rh, red, total; };
__host__ __device__ inline GruLds gru_lds()
{
    GruLds c; Take<int> take;
    c.h = take(kU); c.g = take(2 * kU); c.rh = take(kU); c.red = take(kGruThreads); c.total = take.used;
    return c;
}
__device__ inline float sum4(const float* red, int i) { return (red[i] + red[kU + i]) + (red[2 * kU + i] + red[3 * kU + i]); }

// dot of n (a multiple of 16) register weights with an LDS vector, four chains
template <int n>
__device__ inline float dot_reg(const float (&w)[n], const float* v)
{
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
    const float4* v4 = reinterpret_cast<const float4*>(v);
#pragma unroll
    for (int i = 0; i < n / 4; ++i) {
        const float4 x = v4[i];
        p0 = fmaf(w[4 * i], x.x, p0); p1 = fmaf(w[4 * i + 1], x.y, p1); p2 = fmaf(w[4 * i + 2], x.z, p2); p3 = fmaf(w[4 * i + 3], x.w, p3);
    }
    return (p0 + p1) + (p2 + p3);
}

__global__ void __launch_bounds__(kGruThreads) cg_gru_forward_kernel(GruArgs a)
{
    extern __shared__ float lds[];
    const GruLds c = gru_lds();
    float *hs = lds + c.h, *gs = lds + c.g, *rhs = lds + c.rh, *red = lds + c.red;
    const int n = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, T = a.T;
    // gates: column jg, k in [64 hg, 64 hg + 64); candidate: column jc, k in [32 qc, 32 qc + 32).  A wave shares its k range, so its LDS
    // reads of the state are broadcasts.
    const int jg = (wv >> 1) * 64 + lane, hg = wv & 1, jc = (wv & 1) * 64 + lane, qc = wv >> 1;
    float wg[64], wc[32];
    {
        const float* Wg = a.Wg[dir] + (long long)(kU + 64 * hg) * 2 * kU + jg;
        const float* Wc = a.Wc[dir] + (long long)(kU + 32 * qc) * kU + jc;
#pragma unroll
        for (int i = 0; i < 64; ++i) wg[i] = Wg[i * 2 * kU];
#pragma unroll
        for (int i = 0; i < 32; ++i) wc[i] = Wc[i * kU];
    }
    const int len = a.lengths ? min(max(a.lengths[n], 0), T) : T;
    float *HP = a.HP[dir], *RU = a.RU[dir], *CC = a.CC[dir], *RH = a.RH[dir];
    if (tid < kU) hs[tid] = a.init ? a.init[(long long)n * 2 * kU + dir * kU + tid] : 0.0f;
    lds_barrier();
    for (int s = 0; s < len; ++s) {
        const long long row = (long long)n * T + (dir ? len - 1 - s : s);
        const float gx = tid < 2 * kU ? a.GX[row * 4 * kU + dir * 2 * kU + tid] : 0.0f;
        const float cx = tid < kU ? a.CX[row * 2 * kU + dir * kU + tid] : 0.0f;
        red[hg * 2 * kU + jg] = dot_reg<64>(wg, hs + 64 * hg);
        lds_barrier();
        if (tid < 2 * kU) {
            const float g = sigmoidf_(gx + (red[tid] + red[2 * kU + tid]));
            gs[tid] = g; RU[row * 2 * kU + tid] = g;
            if (tid < kU) rhs[tid] = g * hs[tid];
        }
        lds_barrier();
        red[qc * kU + jc] = dot_reg<32>(wc, rhs + 32 * qc);
        lds_barrier();
        if (tid < kU) {
            const float cc = tanhf(cx + sum4(red, tid)), u = gs[kU + tid], h = hs[tid], hn = u * h + (1.0f - u) * cc;
            HP[row * kU + tid] = h; CC[row * kU + tid] = cc; RH[row * kU + tid] = rhs[tid];
            a.out[row * 2 * kU + dir * kU + tid] = hn;
            hs[tid] = hn;
        }
        lds_barrier();
    }
    // past the length: outputs are zeros (bidirectional_dynamic_rnn), and so is the tape, which the weight products read for every row
    for (int t = len; t < T; ++t) {
        const long long row = (long long)n * T + t;
        if (tid < kU) { a.out[row * 2 * kU + dir * kU + tid] = 0.0f; HP[row * kU + tid] = 0.0f; CC[row * kU + tid] = 0.0f; RH[row * kU + tid] = 0.0f; }
        if (tid < 2 * kU) RU[row * 2 * kU + tid] = 0.0f;
    }
}

// backward through time.  Given dh' : dc~ = dh' (1 - u)(1 - c^2), du~ = dh' (h - c) u (1 - u), d(r h) = W_ch dc~, dr~ = d(r h) h r (1 - r),
// dh = dh' u + d(r h) r + W_gh [dr~ | du~]
__global__ void __launch_bounds__(kGruThreads) cg_gru_backward_kernel(GruArgs a)
{
    extern __shared__ float lds[];
    const GruLds c = gru_lds();
    float *dhs = lds + c.h, *dgs = lds + c.g, *dcs = lds + c.rh, *red = lds + c.red;
    const int n = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, T = a.T;
    // thread (k, q) holds row k of the h rows of both kernels: columns [64 q, 64 q + 64) of gates, [32 q, 32 q + 32) of candidate
    const int k = (wv & 1) * 64 + lane, q = wv >> 1;
    float wg[64], wc[32];
    {
        // (single floats: a tensor's place in the canonical blob is a multiple of 4 bytes, not of 16)
        const float* Wg = a.Wg[dir] + (long long)(kU + k) * 2 * kU + 64 * q;
        const float* Wc = a.Wc[dir] + (long long)(kU + k) * kU + 32 * q;
#pragma unroll
        for (int i = 0; i < 64; ++i) wg[i] = Wg[i];
#pragma unroll
        for (int i = 0; i < 32; ++i) wc[i] = Wc[i];
    }
    const int len = a.lengths ? min(max(a.lengths[n], 0), T) : T;
    const float *HP = a.HP[dir], *RU = a.RU[dir], *CC = a.CC[dir];
    float *DG = a.DG[dir], *DC = a.DC[dir];
    if (tid < kU) dhs[tid] = 0.0f;
    // the tape values of a step are fetched one step ahead
    float nu = 0.0f, nr = 0.0f, ncc = 0.0f, nh = 0.0f, nd = 0.0f;
    auto fetch = [&](int s) {
        if (tid < kU && s < len) {
            const long long row = (long long)n * T + (dir ? s : len - 1 - s);
            nr = RU[row * 2 * kU + tid]; nu = RU[row * 2 * kU + kU + tid]; ncc = CC[row * kU + tid]; nh = HP[row * kU + tid];
            nd = a.dOut[row * 2 * kU + dir * kU + tid];
        }
    };
    fetch(0);
    for (int s = 0; s < len; ++s) {
        const long long row = (long long)n * T + (dir ? s : len - 1 - s);       // the direction's own order, reversed
        const float u = nu, r = nr, cc = ncc, h = nh;
        float dhp = 0.0f;
        if (tid < kU) {
            dhp = dhs[tid] + nd;
            const float dc = dhp * (1.0f - u) * (1.0f - cc * cc), du = dhp * (h - cc) * u * (1.0f - u);
            dcs[tid] = dc; dgs[kU + tid] = du;
            DC[row * kU + tid] = dc; DG[row * 2 * kU + kU + tid] = du;
        }
        fetch(s + 1);
        lds_barrier();
        red[q * kU + k] = dot_reg<32>(wc, dcs + 32 * q);
        lds_barrier();
        float base = 0.0f;
        if (tid < kU) {
            const float drh = sum4(red, tid), dr = drh * h * r * (1.0f - r);
            dgs[tid] = dr; DG[row * 2 * kU + tid] = dr;
            base = dhp * u + drh * r;
        }
        lds_barrier();
        red[q * kU + k] = dot_reg<64>(wg, dgs + 64 * q);
        lds_barrier();
        if (tid < kU) dhs[tid] = base + sum4(red, tid);
    }
    if (a.dinit && tid < kU) a.dinit[(long long)n * 2 * kU + dir * kU + tid] = dhs[tid];
    for (int t = len; t < T; ++t) {
        const long long row = (long long)n * T + t;
        if (tid < kU) DC[row * kU + tid] = 0.0f;
        if (tid < 2 * kU) DG[row * 2 * kU + tid] = 0.0f;
    }
}

}  // namespace cg
using namespace cg;

// ---- the workspace of one handle: ONE carve, which also sizes it
struct CgCarve {
    float *E, *H1, *G1, *X, *G2;                        // encoder: embedded tokens, prenet (outputs and relu gates); X = the CBHG input
    float *bankA, *pool, *A1, *Y1, *A2, *HW0, *hw[9], *Hh[8], *Tg[8], *GX, *CX, *out;
    float *HP[2], *RU[2], *CC[2], *RH[2];
    float *dOut, *DG[2], *DC[2], *dhw, *dhw2, *DHT[8], *dHW0, *dZ2, *dY1, *dZ1, *dpool, *dZb, *dX, *dH1, *dE, *Ds;
    float *wT;                                          // transposed kernels
    double* partial;
};
struct twv_tacotron_cbhg_grad : Handle {
    twv_tacotron_dims d;
    TacoCbhgBlob w;
    int which, N, T, E, P0, F;
    long long wT_floats;
    int lds;                       // bytes, both recurrent kernels
    // the batch norms in the order bank 1 .. K, proj_1, proj_2: channels, the pair's place in the blob, the (4, C) tensor's place in the
    // training vector, the (2, C) piece's place in `pairs` and `stats`
    int n_bn, bn_ch[18];
    long long bn_blob[18], bn_var[18], bn_pair[18], pair_floats;
    int mode = TWV_BN_INFERENCE;   // twv_tacotron_cbhg_grad_set_mode
    const float* variables = nullptr;      // batch mode: the caller's training vector (gamma and beta are read from it at every forward)
    float *pairs = nullptr, *stats = nullptr;       // batch mode: the handle's own device buffers, pair_floats each
    int forwarded = 0, has_bh = 0, has_init = 0;    // a forward has been made since create / set_mode, with these optional inputs
    ~twv_tacotron_cbhg_grad()
    {
        if (pairs) (void)hipFree(pairs);
        if (stats) (void)hipFree(stats);
    }
};
using Cg = twv_tacotron_cbhg_grad;

static long long cg_carve(const twv_tacotron_cbhg_grad* g, float* base, CgCarve& c)
{
    const TacoCbhgBlob& w = g->w;
    const long long rows = (long long)g->N * g->T;
    const int CB = w.bank * w.bch, Cin = w.Cin, P0 = w.proj[0], P1 = w.proj[1];
    TakeFloats take{base};
    memset(&c, 0, sizeof(c));
    if (g->which == 0) {
        c.E = take(rows * g->E); c.H1 = take(rows * g->P0); c.G1 = take(rows * g->P0); c.X = take(rows * Cin); c.G2 = take(rows * Cin);
        c.dH1 = take(rows * g->P0); c.dE = take(rows * g->E);
    }
    c.bankA = take(rows * CB); c.pool = take(rows * CB); c.A1 = take(rows * P0); c.Y1 = take(rows * P0); c.A2 = take(rows * P1); c.HW0 = take(rows * P1);
    for (int i = 0; i <= w.depth; ++i) c.hw[i] = (i == 0 && !w.has_dense) ? c.HW0 : take(rows * kU);
    for (int i = 0; i < w.depth; ++i) { c.Hh[i] = take(rows * kU); c.Tg[i] = take(rows * kU); c.DHT[i] = take(rows * 2 * kU); }
    c.GX = take(rows * 4 * kU); c.CX = take(rows * 2 * kU); c.out = take(rows * 2 * kU);
    for (int dr = 0; dr < 2; ++dr) {
        c.HP[dr] = take(rows * kU); c.RU[dr] = take(rows * 2 * kU); c.CC[dr] = take(rows * kU); c.RH[dr] = take(rows * kU);
        c.DG[dr] = take(rows * 2 * kU); c.DC[dr] = take(rows * kU);
    }
    c.dOut = take(rows * 2 * kU); c.dhw = take(rows * kU); c.dhw2 = take(rows * kU); c.dHW0 = take(rows * P1); c.dZ2 = take(rows * P1);
    c.dY1 = take(rows * P0); c.dZ1 = take(rows * P0); c.dpool = take(rows * CB); c.dZb = take(rows * CB); c.dX = take(rows * Cin);
    int widest = w.bch > P0 ? w.bch : P0; widest = widest > P1 ? widest : P1;
    c.Ds = take(rows * widest);
    c.wT = take(g->wT_floats);
    const long long nchunk = (rows + kChunk - 1) / kChunk;
    int cmax = 2 * kU;                                  // the widest matrix a column-statistics kernel is run on
    for (int v : {CB, P0, P1, Cin, g->P0, g->F, g->E}) cmax = cmax > v ? cmax : v;
    c.partial = reinterpret_cast<double*>(take((nchunk * 2 + 2) * cmax * 2));      // (every piece starts at a multiple of four floats; + the batch mode's two coefficient rows)
    return take.off.used;
}

static const char* const kCgBuilt = "the CBHG gradient is built for single-speaker and 'deepvoice' models, enc_rnn_size = post_rnn_size = 128 and projection widths up to 16";

// what _create and _reshape accept of (which, batch, t) for the model `d`: one validation, the same codes and words from both
static int cg_check_sizes(const twv_tacotron_dims& d, int which, int batch, int t)
{
    if (which != TWV_CBHG_ENCODER && which != TWV_CBHG_POST) return twv_fail(TWV_E_INVALID, "which must be TWV_CBHG_ENCODER (0) or TWV_CBHG_POST (1)");
    if (batch < 1) return twv_fail(TWV_E_INVALID, "batch >= 1 required");
    if (which == TWV_CBHG_ENCODER && (t < 1 || t > 1024)) return twv_fail(TWV_E_INVALID, "encoder: 1 <= t_in <= 1024 required");
    if (which == TWV_CBHG_POST && (t < 1 || t > d.max_iters * d.reduction_factor)) return twv_fail(TWV_E_INVALID, "post net: 1 <= t_out <= max_iters * r required");
    if ((long long)batch * t > (1LL << 24)) return twv_fail(TWV_E_INVALID, "batch * t above 2^24 rows");
    if (d.num_speakers > 1 && d.model_simple && d.speaker_embedding_size != 1)
        return twv_fail(TWV_E_UNSUPPORTED, std::string("model_type 'simple': ") + kCgBuilt);
    return TWV_OK;
}

extern "C" int twv_tacotron_cbhg_grad_create(const twv_tacotron* h, int which, int batch, int t, twv_tacotron_cbhg_grad** out)
{
    if (!h || !out) return twv_fail(TWV_E_INVALID, "null argument");
    const twv_tacotron_dims& d = taco_dims(h);
    GRAD_CHK(cg_check_sizes(d, which, batch, t));
    twv_tacotron_cbhg_grad* g = new twv_tacotron_cbhg_grad();
    g->d = d; g->which = which; g->N = batch; g->T = t;
    taco_cbhg_blob(h, which, g->w);
    const TacoCbhgBlob& w = g->w;
    // the row kernel stages kRB + kw - 1 rows of a K chunk: convolutions up to kMaxKw wide (the bank's are bounded by twv_tacotron_create)
    if (w.pw < 1 || w.pw > kMaxKw || w.bank > kMaxKw || w.rnn != kU) {
        delete g;
        return twv_fail(TWV_E_UNSUPPORTED, std::string("proj_width above 16: ") + kCgBuilt);
    }
    {
        long long ahead = 0, poff = 0;
        if (which == TWV_CBHG_POST) {       // the encoder's batch norms lie in front of the post net's in the training vector
            TacoCbhgBlob e;
            taco_cbhg_blob(h, TWV_CBHG_ENCODER, e);
            ahead = 2LL * ((long long)e.bank * e.bch + e.proj[0] + e.proj[1]);
        }
        g->n_bn = w.bank + 2;
        for (int i = 0; i < g->n_bn; ++i) {
            g->bn_ch[i] = i < w.bank ? w.bch : w.proj[i - w.bank];
            g->bn_blob[i] = i < w.bank ? w.bn[i + 1] : w.pbn[i - w.bank];
            g->bn_var[i] = g->bn_blob[i] + ahead; ahead += 2LL * g->bn_ch[i];
            g->bn_pair[i] = poff; poff += 2LL * g->bn_ch[i];
        }
        g->pair_floats = poff;
    }
    g->E = which ? 0 : d.embedding_size; g->P0 = which ? 0 : d.enc_prenet_sizes[0]; g->F = which ? d.num_freq : 0;
    const int CB = w.bank * w.bch;
    long long wt = 0;
    for (int k = 1; k <= w.bank; ++k) wt += (long long)k * w.Cin * w.bch;
    wt += (long long)w.pw * CB * w.proj[0] + (long long)w.pw * w.proj[0] * w.proj[1] + (w.has_dense ? (long long)w.proj[1] * kU : 0);
    wt += (long long)w.depth * 2 * kU * kU + 2LL * (2 * kU * kU + kU * kU);
    if (which) wt += (long long)2 * kU * d.num_freq; else wt += (long long)d.enc_prenet_sizes[0] * d.enc_prenet_sizes[1] + (long long)d.embedding_size * d.enc_prenet_sizes[0];
    g->wT_floats = wt + 64;
    CgCarve c;
    g->ws_floats = cg_carve(g, nullptr, c);
    g->lds = gru_lds().total * 4;
    g->route = std::string("kernel=cg_bigru side=") + (which ? "post" : "encoder") + " workgroups_per_utterance=2 threads=512 weights=registers bank=" +
               std::to_string(w.bank) + " bank_channels=" + std::to_string(w.bch) + " highway=" + std::to_string(w.depth) + " dense=" +
               std::to_string(w.has_dense) + " lds=" + std::to_string(g->lds) + " wgrad=rocblas";
    *out = g;
    return TWV_OK;
}
// The handle at another (batch, t): what a _create at these sizes followed by the handle's set_mode would give.  Kept: the rocBLAS handle,
// the events and the timing flag, the batch-norm mode and its variables pointer, and `pairs` / `stats` -- pair_floats is a sum of channel
// counts (bank * bank channels + the two projection widths, twice), as is wT_floats, so neither follows the sizes; every forward in batch
// mode writes all of `pairs` and `stats` before it reads them.  The label carries no sizes.  A refused call leaves the handle as it was.
extern "C" int twv_tacotron_cbhg_grad_reshape(twv_tacotron_cbhg_grad* g, int batch, int t)
{
    if (!g) return twv_fail(TWV_E_INVALID, "null argument");
    GRAD_CHK(cg_check_sizes(g->d, g->which, batch, t));
    g->N = batch; g->T = t;
    CgCarve c;
    g->ws_floats = cg_carve(g, nullptr, c);
    g->forwarded = 0; g->has_bh = 0; g->has_init = 0;
    return TWV_OK;
}
extern "C" void twv_tacotron_cbhg_grad_destroy(twv_tacotron_cbhg_grad* g) { delete g; }
extern "C" int twv_tacotron_cbhg_grad_set_timing(twv_tacotron_cbhg_grad* g, int on) { return g ? g->set_timing(on) : twv_fail(TWV_E_INVALID, "null argument"); }
extern "C" size_t twv_tacotron_cbhg_grad_workspace_bytes(const twv_tacotron_cbhg_grad* g) { return g ? (size_t)g->ws_floats * 4 : 0; }
extern "C" const char* twv_tacotron_cbhg_grad_route(const twv_tacotron_cbhg_grad* g) { return g ? g->route.c_str() : ""; }
extern "C" int twv_tacotron_cbhg_grad_set_mode(twv_tacotron_cbhg_grad* g, int mode, const float* variables)
{
    if (!g) return twv_fail(TWV_E_INVALID, "null argument");
    if (mode != TWV_BN_INFERENCE && mode != TWV_BN_BATCH) return twv_fail(TWV_E_INVALID, "mode must be TWV_BN_INFERENCE (0) or TWV_BN_BATCH (1)");
    if (mode == TWV_BN_BATCH && !variables) return twv_fail(TWV_E_INVALID, "batch mode needs the training vector (gamma and beta are read from it)");
    if (mode == TWV_BN_BATCH && !g->pairs) {
        GRAD_HIPCHK(hipMalloc(&g->pairs, (size_t)g->pair_floats * 4));
        GRAD_HIPCHK(hipMalloc(&g->stats, (size_t)g->pair_floats * 4));
    }
    g->mode = mode; g->variables = mode == TWV_BN_BATCH ? variables : nullptr; g->forwarded = 0;
    return TWV_OK;
}
extern "C" size_t twv_tacotron_cbhg_grad_batch_stats_floats(const twv_tacotron_cbhg_grad* g) { return g ? (size_t)g->pair_floats : 0; }
extern "C" int twv_tacotron_cbhg_grad_batch_stats(const twv_tacotron_cbhg_grad* g, float* out, void* stream)
{
    if (!g || !out) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->mode != TWV_BN_BATCH || !g->forwarded) return twv_fail(TWV_E_INVALID, "batch statistics: no forward in batch mode has been made on this handle");
    GRAD_HIPCHK(hipMemcpyAsync(out, g->stats, (size_t)g->pair_floats * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TWV_OK;
}

namespace {

// one run's launches: the stream, the sizes and the helpers the encoder and the post net share
struct CgRun {
    twv_tacotron_cbhg_grad* g;
    hipStream_t st;
    const float* blob;
    float* grad;
    CgCarve c;
    int rows, T;
    long long wt_used = 0;

    RowsArgs rows_args(const float* X, int ldx, int Cin, int kw, int left, const float* W, int ldw, int ncols, const float* bias) const
    {
        return tgrad::rows_args(X, ldx, rows, T, Cin, kw, left, W, ldw, ncols, bias);
    }
    void launch(const RowsArgs& a) const { launch_rows<Cg>(st, a); }
    // C (ldc) = (add ? C : 0) + D (rows x ncols, ldd) (*) W^T: the backward of a convolution / dense layer W (kw, Cin, ncols; row stride ldw)
    // with respect to its input.  The transposed, tap-reversed kernel is laid down in the workspace first.
    void data_grad(const float* D, int ldd, int ncols, const float* W, int ldw, int Cin, int kw, float* C, int ldc, int add, const float* gate_in = nullptr)
    {
        float* Wt = c.wT + wt_used;
        wt_used += (long long)kw * Cin * ncols;
        hipLaunchKernelGGL(cg_transpose_kernel, dim3(grid_for((long long)kw * Cin * ncols)), dim3(256), 0, st, W, kw, Cin, ncols, ldw, Wt);
        RowsArgs a = rows_args(D, ldd, ncols, kw, (kw - 1) - (kw - 1) / 2, Wt, Cin, Cin, nullptr);
        a.C = C; a.ldc = ldc; a.add = add; a.gate_in = gate_in;
        launch(a);
    }
    // the kernel gradient of a convolution: tap by tap, dW[tap] = X[r + tap - left]^T . D[r] over the rows whose shifted row lies in the same
    // utterance (the others are zeroed in a copy of D)
    int conv_wgrad(const float* X, int ldx, int Cin, const float* D, int ldd, int Nc, int kw, long long off) const
    {
        const int left = (kw - 1) / 2;
        for (int tap = 0; tap < kw; ++tap) {
            const int s = tap - left;
            const long long o = off + (long long)tap * Cin * Nc;
            if (s <= -T || s >= T) { GRAD_HIPCHK(hipMemsetAsync(grad + o, 0, (size_t)Cin * Nc * 4, st)); continue; }
            const float* Dp = D; int ld = ldd;
            if (s != 0) {
                hipLaunchKernelGGL(cg_shift_mask_kernel, dim3(grid_for((long long)rows * Nc)), dim3(256), 0, st, D, ldd, rows, T, Nc, s, c.Ds);
                Dp = c.Ds; ld = Nc;
            }
            const long long n = rows - (s < 0 ? -s : s);
            GRAD_CHK(s >= 0 ? g->wgrad(X + (long long)s * ldx, ldx, Cin, Dp, ld, Nc, o, n) : g->wgrad(X, ldx, Cin, Dp + (long long)(-s) * ld, ld, Nc, o, n));
        }
        return TWV_OK;
    }
    void colsum(const float* D, int ld, int Nc, long long off) const
    {
        const int nchunk = (rows + kChunk - 1) / kChunk;
        hipLaunchKernelGGL(cg_colsum_kernel, dim3((Nc + 63) / 64, nchunk), dim3(256), 0, st, D, ld, rows, Nc, c.partial);
        FinishArgs f;
        memset(&f, 0, sizeof(f));
        f.off[0][0] = off; f.gs = Nc; f.nstat = 1; f.Cn = Nc; f.nchunk = nchunk;
        hipLaunchKernelGGL(cg_finish_kernel, dim3((Nc + 63) / 64), dim3(64), 0, st, c.partial, f, grad);
    }
    bool batch() const { return g->mode == TWV_BN_BATCH; }
    // the handle's batch norms first .. first + n - 1 (gs channels each) as the groups of one launch: their pairs in the blob (and so in
    // the gradient), or, in_pairs, in the handle's own `pairs`
    Groups groups(int first, int n, int gs, bool in_pairs) const
    {
        Groups gr;
        memset(&gr, 0, sizeof(gr));
        gr.gs = gs;
        for (int q = 0; q < n; ++q) { gr.inv[q] = in_pairs ? g->bn_pair[first + q] : g->bn_blob[first + q]; gr.shift[q] = gr.inv[q] + gs; }
        return gr;
    }
    BatchGroups batch_groups(int first, int n, int gs) const
    {
        BatchGroups b;
        memset(&b, 0, sizeof(b));
        b.gs = gs;
        for (int q = 0; q < n; ++q) { b.pair[q] = g->bn_pair[first + q]; b.var[q] = g->bn_var[first + q]; }
        return b;
    }
    // what a kernel reads a batch norm's (inv, shift) from: the blob, or the batch pairs
    const float* bn_base() const { return batch() ? g->pairs : blob; }
    Groups bn_read(int first, int n, int gs) const { return groups(first, n, gs, batch()); }
    // batch mode: the statistics of A's columns over all rows and the pairs derived from them
    void batch_stats(const float* A, int lda, int first, int n, int gs, int Cn) const
    {
        const int nchunk = (rows + kChunk - 1) / kChunk;
        hipLaunchKernelGGL(cg_stats_kernel, dim3((Cn + 63) / 64, nchunk), dim3(256), 0, st, A, lda, rows, Cn, c.partial);
        hipLaunchKernelGGL(cg_stats_finish_kernel, dim3((Cn + 63) / 64), dim3(64), 0, st, c.partial, batch_groups(first, n, gs), Cn, nchunk, rows,
                           g->variables, g->stats, g->pairs);
    }
    // dZ = batch norm / relu (/ max pool) backward of dY against the tape A.  Inference mode: the (d_inv, d_shift) pairs land in the groups'
    // blob slots; batch mode: (d_gamma, d_beta) do, and dZ is the backward through the statistics too
    void bn_bwd(const float* dY, int ldy, const float* A, int lda, int first, int n, int gs, int Cn, int pool, int relu, float* dZ, int ldz) const
    {
        const int nchunk = (rows + kChunk - 1) / kChunk;
        const Groups gr = groups(first, n, gs, false);
        if (batch()) {
            const BatchGroups b = batch_groups(first, n, gs);
            double* coef = c.partial + (long long)nchunk * 2 * Cn;
            hipLaunchKernelGGL(cg_bn_batch_sums_kernel, dim3((Cn + 63) / 64, nchunk), dim3(256), 0, st, dY, ldy, A, lda, g->pairs, groups(first, n, gs, true),
                               rows, T, Cn, pool, dZ, ldz, c.partial);
            hipLaunchKernelGGL(cg_bn_batch_finish_kernel, dim3((Cn + 63) / 64), dim3(64), 0, st, c.partial, b, gr, Cn, nchunk, rows, g->stats, coef, grad);
            hipLaunchKernelGGL(cg_bn_batch_bwd_kernel, dim3(grid_for((long long)rows * Cn)), dim3(256), 0, st, dZ, ldz, A, lda, g->pairs, g->stats, b, coef,
                               rows, Cn, relu);
            return;
        }
        hipLaunchKernelGGL(cg_bn_bwd_kernel, dim3((Cn + 63) / 64, nchunk), dim3(256), 0, st, dY, ldy, A, lda, blob, gr, rows, T, Cn, pool, relu, dZ, ldz, c.partial);
        FinishArgs f;
        memset(&f, 0, sizeof(f));
        for (int q = 0; q < 17; ++q) { f.off[0][q] = gr.inv[q]; f.off[1][q] = gr.shift[q]; }
        f.gs = gr.gs; f.nstat = 2; f.Cn = Cn; f.nchunk = nchunk;
        hipLaunchKernelGGL(cg_finish_kernel, dim3((Cn + 63) / 64), dim3(64), 0, st, c.partial, f, grad);
    }
};

// the CBHG forward from r.c.X-or-`x` (rows x Cin) to r.c.out, recording; `bh` (N, proj[1]) and `init` (N, 2 kU) may be null
int cbhg_forward(CgRun& r, const float* x, const float* bh, const float* init, const int32_t* lengths)
{
    const TacoCbhgBlob& w = r.g->w;
    const CgCarve& c = r.c;
    const float* B = r.blob;
    const int Cin = w.Cin, CB = w.bank * w.bch, P0 = w.proj[0], P1 = w.proj[1], pl = (w.pw - 1) / 2;
    const long long rows = r.rows;
    const bool batch = r.batch();
    for (int k = 1; k <= w.bank; ++k) {
        RowsArgs a = r.rows_args(x, Cin, Cin, k, (k - 1) / 2, B + w.W[k], w.bch, w.bch, B + w.b[k]);
        a.act = 1; a.C = c.bankA + (long long)(k - 1) * w.bch; a.ldc = CB;
        r.launch(a);
    }
    if (batch) r.batch_stats(c.bankA, CB, 0, w.bank, w.bch, CB);
    hipLaunchKernelGGL(cg_pool_kernel, dim3(grid_for(rows * CB)), dim3(256), 0, r.st, c.bankA, r.bn_base(), r.bn_read(0, w.bank, w.bch), r.rows, r.T, CB, c.pool);
    // In batch mode a projection's batch norm cannot ride in the row kernel (the statistics need all of A): rows, statistics, apply
    {
        RowsArgs a = r.rows_args(c.pool, CB, CB, w.pw, pl, B + w.pW[0], P0, P0, B + w.pb[0]);
        a.act = 1; a.C = c.A1; a.ldc = P0;
        if (!batch) { a.Y = c.Y1; a.ldy = P0; a.inv = B + w.pbn[0]; a.shift = B + w.pbn[0] + P0; }
        r.launch(a);
        if (batch) {
            r.batch_stats(c.A1, P0, w.bank, 1, P0, P0);
            const float* pr = r.g->pairs + r.g->bn_pair[w.bank];
            hipLaunchKernelGGL(cg_bn_apply_kernel, dim3(grid_for(rows * P0)), dim3(256), 0, r.st, c.A1, pr, pr + P0, (const float*)nullptr, 0,
                               (const float*)nullptr, 0, r.rows, r.T, P0, c.Y1);
        }
    }
    {   // second projection + residual: (proj + inputs) + before_highway
        RowsArgs a = r.rows_args(c.Y1, P0, P0, w.pw, pl, B + w.pW[1], P1, P1, B + w.pb[1]);
        a.C = c.A2; a.ldc = P1;
        if (!batch) {
            a.Y = c.HW0; a.ldy = P1; a.inv = B + w.pbn[1]; a.shift = B + w.pbn[1] + P1;
            a.add1 = x; a.ld1 = Cin; a.add2 = bh; a.ld2 = P1;
        }
        r.launch(a);
        if (batch) {
            r.batch_stats(c.A2, P1, w.bank + 1, 1, P1, P1);
            const float* pr = r.g->pairs + r.g->bn_pair[w.bank + 1];
            hipLaunchKernelGGL(cg_bn_apply_kernel, dim3(grid_for(rows * P1)), dim3(256), 0, r.st, c.A2, pr, pr + P1, x, Cin, bh, P1, r.rows, r.T, P1, c.HW0);
        }
    }
    if (w.has_dense) {
        RowsArgs a = r.rows_args(c.HW0, P1, P1, 1, 0, B + w.dW, kU, kU, B + w.db);
        a.C = c.hw[0]; a.ldc = kU;
        r.launch(a);
    }
    for (int i = 0; i < w.depth; ++i) {
        RowsArgs a = r.rows_args(c.hw[i], kU, kU, 1, 0, B + w.hH[i], kU, kU, B + w.hHb[i]);
        a.act = 1; a.C = c.Hh[i]; a.ldc = kU;
        r.launch(a);
        a = r.rows_args(c.hw[i], kU, kU, 1, 0, B + w.hT[i], kU, kU, B + w.hTb[i]);
        a.act = 2; a.C = c.Tg[i]; a.ldc = kU;
        r.launch(a);
        hipLaunchKernelGGL(cg_highway_kernel, dim3(grid_for(rows * kU)), dim3(256), 0, r.st, c.hw[i], c.Hh[i], c.Tg[i], rows * kU, c.hw[i + 1]);
    }
    const float* top = c.hw[w.depth];
    for (int dr = 0; dr < 2; ++dr) {      // the input halves of both GRU kernels, all rows at once
        RowsArgs a = r.rows_args(top, kU, kU, 1, 0, B + w.gWg[dr], 2 * kU, 2 * kU, B + w.gbg[dr]);
        a.C = c.GX + dr * 2 * kU; a.ldc = 4 * kU;
        r.launch(a);
        a = r.rows_args(top, kU, kU, 1, 0, B + w.gWc[dr], kU, kU, B + w.gbc[dr]);
        a.C = c.CX + dr * kU; a.ldc = 2 * kU;
        r.launch(a);
    }
    GruArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int dr = 0; dr < 2; ++dr) {
        ga.Wg[dr] = B + w.gWg[dr]; ga.Wc[dr] = B + w.gWc[dr];
        ga.HP[dr] = c.HP[dr]; ga.RU[dr] = c.RU[dr]; ga.CC[dr] = c.CC[dr]; ga.RH[dr] = c.RH[dr]; ga.DG[dr] = c.DG[dr]; ga.DC[dr] = c.DC[dr];
    }
    ga.GX = c.GX; ga.CX = c.CX; ga.init = init; ga.lengths = lengths; ga.out = c.out; ga.N = r.g->N; ga.T = r.T;
    hipLaunchKernelGGL(cg_gru_forward_kernel, dim3(2 * r.g->N), dim3(kGruThreads), (size_t)r.g->lds, r.st, ga);
    return TWV_OK;
}

// the CBHG backward from r.c.dOut (rows x 2 kU) to r.c.dX (rows x Cin); phases: marks 1 .. 2 the GRUs, 2 .. 3 the row-wise backward
int cbhg_backward_data(CgRun& r, const int32_t* lengths, float* d_bh, float* d_init)
{
    const TacoCbhgBlob& w = r.g->w;
    const CgCarve& c = r.c;
    const float* B = r.blob;
    const int Cin = w.Cin, CB = w.bank * w.bch, P0 = w.proj[0], P1 = w.proj[1];
    const long long rows = r.rows;
    GruArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int dr = 0; dr < 2; ++dr) {
        ga.Wg[dr] = B + w.gWg[dr]; ga.Wc[dr] = B + w.gWc[dr];
        ga.HP[dr] = c.HP[dr]; ga.RU[dr] = c.RU[dr]; ga.CC[dr] = c.CC[dr]; ga.RH[dr] = c.RH[dr]; ga.DG[dr] = c.DG[dr]; ga.DC[dr] = c.DC[dr];
    }
    ga.lengths = lengths; ga.dOut = c.dOut; ga.dinit = d_init; ga.N = r.g->N; ga.T = r.T;
    hipLaunchKernelGGL(cg_gru_backward_kernel, dim3(2 * r.g->N), dim3(kGruThreads), (size_t)r.g->lds, r.st, ga);
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(r.g->mark(2));
    // dx = delta . W_x^T of both kernels and both directions, products over all rows
    float* dcur = (w.depth & 1) ? c.dhw2 : c.dhw;       // (ping-pong so that the bottom of the highway stack lands in c.dhw)
    for (int dr = 0; dr < 2; ++dr) {
        r.data_grad(c.DG[dr], 2 * kU, 2 * kU, B + w.gWg[dr], 2 * kU, kU, 1, dcur, kU, dr);
        r.data_grad(c.DC[dr], kU, kU, B + w.gWc[dr], kU, kU, 1, dcur, kU, 1);
    }
    for (int i = w.depth - 1; i >= 0; --i) {
        float* dnext = dcur == c.dhw ? c.dhw2 : c.dhw;
        hipLaunchKernelGGL(cg_highway_bwd_kernel, dim3(grid_for(rows * kU)), dim3(256), 0, r.st, dcur, c.hw[i], c.Hh[i], c.Tg[i], rows * kU, c.DHT[i], dnext);
        r.data_grad(c.DHT[i], 2 * kU, kU, B + w.hH[i], kU, kU, 1, dnext, kU, 1);
        r.data_grad(c.DHT[i] + kU, 2 * kU, kU, B + w.hT[i], kU, kU, 1, dnext, kU, 1);
        dcur = dnext;
    }
    // dcur == c.dhw: the cotangent of the highway stack's input
    const float* dHW0 = c.dhw;
    if (w.has_dense) { r.data_grad(c.dhw, kU, kU, B + w.dW, kU, P1, 1, c.dHW0, P1, 0); dHW0 = c.dHW0; }
    if (d_bh) hipLaunchKernelGGL(cg_utterance_sum_kernel, dim3((r.g->N * P1 + 255) / 256), dim3(256), 0, r.st, dHW0, r.g->N, r.T, P1, d_bh);
    r.bn_bwd(dHW0, P1, c.A2, P1, w.bank + 1, 1, P1, P1, 0, 0, c.dZ2, P1);
    r.data_grad(c.dZ2, P1, P1, B + w.pW[1], P1, P0, w.pw, c.dY1, P0, 0);
    r.bn_bwd(c.dY1, P0, c.A1, P0, w.bank, 1, P0, P0, 0, 1, c.dZ1, P0);
    r.data_grad(c.dZ1, P0, P0, B + w.pW[0], P0, CB, w.pw, c.dpool, CB, 0);
    r.bn_bwd(c.dpool, CB, c.bankA, CB, 0, w.bank, w.bch, CB, 1, 1, c.dZb, CB);
    // d_x: the residual's share, then the bank's convolutions in order
    GRAD_HIPCHK(hipMemcpy2DAsync(c.dX, (size_t)Cin * 4, dHW0, (size_t)P1 * 4, (size_t)Cin * 4, (size_t)rows, hipMemcpyDeviceToDevice, r.st));
    for (int k = 1; k <= w.bank; ++k) r.data_grad(c.dZb + (long long)(k - 1) * w.bch, CB, w.bch, B + w.W[k], w.bch, Cin, k, c.dX, Cin, 1);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

// every kernel / bias gradient of the CBHG from the tape and the deltas
int cbhg_weight_grads(CgRun& r, const float* x)
{
    const TacoCbhgBlob& w = r.g->w;
    const CgCarve& c = r.c;
    const int Cin = w.Cin, CB = w.bank * w.bch, P0 = w.proj[0], P1 = w.proj[1];
    const long long rows = r.rows;
    const float* top = c.hw[w.depth];
    for (int dr = 0; dr < 2; ++dr) {
        GRAD_CHK(r.g->wgrad(top, kU, kU, c.DG[dr], 2 * kU, 2 * kU, w.gWg[dr], rows));
        GRAD_CHK(r.g->wgrad(c.HP[dr], kU, kU, c.DG[dr], 2 * kU, 2 * kU, w.gWg[dr] + (long long)kU * 2 * kU, rows));
        r.colsum(c.DG[dr], 2 * kU, 2 * kU, w.gbg[dr]);
        GRAD_CHK(r.g->wgrad(top, kU, kU, c.DC[dr], kU, kU, w.gWc[dr], rows));
        GRAD_CHK(r.g->wgrad(c.RH[dr], kU, kU, c.DC[dr], kU, kU, w.gWc[dr] + (long long)kU * kU, rows));
        r.colsum(c.DC[dr], kU, kU, w.gbc[dr]);
    }
    for (int i = 0; i < w.depth; ++i) {
        GRAD_CHK(r.g->wgrad(c.hw[i], kU, kU, c.DHT[i], 2 * kU, kU, w.hH[i], rows)); r.colsum(c.DHT[i], 2 * kU, kU, w.hHb[i]);
        GRAD_CHK(r.g->wgrad(c.hw[i], kU, kU, c.DHT[i] + kU, 2 * kU, kU, w.hT[i], rows)); r.colsum(c.DHT[i] + kU, 2 * kU, kU, w.hTb[i]);
    }
    if (w.has_dense) { GRAD_CHK(r.g->wgrad(c.HW0, P1, P1, c.dhw, kU, kU, w.dW, rows)); r.colsum(c.dhw, kU, kU, w.db); }
    GRAD_CHK(r.conv_wgrad(c.Y1, P0, P0, c.dZ2, P1, P1, w.pw, w.pW[1])); r.colsum(c.dZ2, P1, P1, w.pb[1]);
    GRAD_CHK(r.conv_wgrad(c.pool, CB, CB, c.dZ1, P0, P0, w.pw, w.pW[0])); r.colsum(c.dZ1, P0, P0, w.pb[0]);
    for (int k = 1; k <= w.bank; ++k) {
        const float* D = c.dZb + (long long)(k - 1) * w.bch;
        GRAD_CHK(r.conv_wgrad(x, Cin, Cin, D, CB, w.bch, k, w.W[k])); r.colsum(D, CB, w.bch, w.b[k]);
    }
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

int cg_begin(twv_tacotron_cbhg_grad* g, CgRun& r, const float* blob, void* workspace, int32_t* status, void* stream, float* grad_blob)
{
    r.g = g; r.st = (hipStream_t)stream; r.blob = blob; r.grad = grad_blob; r.rows = g->N * g->T; r.T = g->T;
    if (g->mode == TWV_BN_BATCH && (!g->variables || !g->pairs)) return twv_fail(TWV_E_INVALID, "batch mode without a training vector (twv_tacotron_cbhg_grad_set_mode)");
    GRAD_CHK(g->begin(r.st, status, grad_blob, g->w.blob_floats));       // (a forward has no gradient to zero: grad_blob null)
    cg_carve(g, (float*)workspace, r.c);
    GRAD_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(cg_gru_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, g->lds));
    GRAD_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(cg_gru_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, g->lds));
    return TWV_OK;
}

}  // namespace

// ---- the two halves of a pass.  The tape of a forward stays in the caller's workspace until the handle's next forward; a backward reads
// it, so it is given the same workspace (and the same blob and inputs).
extern "C" int twv_tacotron_encoder_grad_forward(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                                 const float* before_highway, const float* rnn_init, const float* mask1, const float* mask2,
                                                 void* workspace, int32_t* status, void* stream, float* memory_out)
{
    if (!g || !blob || !tokens || !lengths || !workspace || !status || !memory_out) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_ENCODER) return twv_fail(TWV_E_INVALID, "the handle was created for the post net");
    CgRun r;
    GRAD_CHK(cg_begin(g, r, blob, workspace, status, stream, nullptr));
    const TacoCbhgBlob& w = g->w;
    const CgCarve& c = r.c;
    const int E = g->E, P0 = g->P0, P1 = w.Cin, rows = r.rows;
    // ---- (a) recording forward
    GRAD_CHK(r.g->mark(0));
    hipLaunchKernelGGL(cg_embed_kernel, dim3(grid_for((long long)rows * E)), dim3(256), 0, r.st, blob + w.emb, tokens, rows, E, g->d.n_symbols, c.E);
    {
        RowsArgs a = r.rows_args(c.E, E, E, 1, 0, blob + w.pW1, P0, P0, blob + w.pb1);
        a.act = 1; a.mask = mask1; a.gate_out = c.G1; a.C = c.H1; a.ldc = P0;
        r.launch(a);
        a = r.rows_args(c.H1, P0, P0, 1, 0, blob + w.pW2, P1, P1, blob + w.pb2);
        a.act = 1; a.mask = mask2; a.gate_out = c.G2; a.C = c.X; a.ldc = P1;
        r.launch(a);
    }
    GRAD_CHK(cbhg_forward(r, c.X, before_highway, rnn_init, lengths));
    GRAD_HIPCHK(hipMemcpyAsync(memory_out, c.out, (size_t)rows * 2 * kU * 4, hipMemcpyDeviceToDevice, r.st));
    GRAD_HIPCHK(hipGetLastError());
    g->forwarded = 1; g->has_bh = before_highway ? 1 : 0; g->has_init = rnn_init ? 1 : 0;
    return TWV_OK;
}

extern "C" int twv_tacotron_encoder_grad_backward(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                                  const float* d_memory, void* workspace, int32_t* status, void* stream, float* grad_blob,
                                                  float* d_before_highway, float* d_rnn_init)
{
    if (!g || !blob || !tokens || !lengths || !d_memory || !workspace || !status || !grad_blob) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_ENCODER) return twv_fail(TWV_E_INVALID, "the handle was created for the post net");
    if (!g->forwarded) return twv_fail(TWV_E_INVALID, "backward: no forward has been made on this handle (twv_tacotron_encoder_grad_forward)");
    if ((g->has_bh && !d_before_highway) || (g->has_init && !d_rnn_init)) return twv_fail(TWV_E_INVALID, "null argument: before_highway / rnn_init need their d_ outputs");
    CgRun r;
    GRAD_CHK(cg_begin(g, r, blob, workspace, status, stream, grad_blob));
    const TacoCbhgBlob& w = g->w;
    const CgCarve& c = r.c;
    const int E = g->E, P0 = g->P0, P1 = w.Cin, rows = r.rows;
    // ---- (b) the GRUs backward through time, (c) the row-wise backward
    GRAD_CHK(r.g->mark(1));
    GRAD_HIPCHK(hipMemcpyAsync(c.dOut, d_memory, (size_t)rows * 2 * kU * 4, hipMemcpyDeviceToDevice, r.st));
    GRAD_CHK(cbhg_backward_data(r, lengths, g->has_bh ? d_before_highway : nullptr, g->has_init ? d_rnn_init : nullptr));
    launch_mul<Cg>(r.st, c.dX, c.G2, (long long)rows * P1);
    r.data_grad(c.dX, P1, P1, blob + w.pW2, P1, P0, 1, c.dH1, P0, 0, c.G1);
    r.data_grad(c.dH1, P0, P0, blob + w.pW1, P0, E, 1, c.dE, E, 0);
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(r.g->mark(3));
    // ---- (d) weight gradients
    GRAD_CHK(cbhg_weight_grads(r, c.X));
    GRAD_CHK(r.g->wgrad(c.H1, P0, P0, c.dX, P1, P1, w.pW2, rows)); r.colsum(c.dX, P1, P1, w.pb2);
    GRAD_CHK(r.g->wgrad(c.E, E, E, c.dH1, P0, P0, w.pW1, rows)); r.colsum(c.dH1, P0, P0, w.pb1);
    hipLaunchKernelGGL(cg_embed_grad_kernel, dim3(g->d.n_symbols), dim3(256), 0, r.st, c.dE, tokens, rows, E, grad_blob + w.emb);
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(r.g->mark(4));
    return TWV_OK;
}

// forward, then backward, in the handle's mode
extern "C" int twv_tacotron_encoder_grad_run(twv_tacotron_cbhg_grad* g, const float* blob, const int32_t* tokens, const int32_t* lengths,
                                             const float* before_highway, const float* rnn_init, const float* mask1, const float* mask2,
                                             const float* d_memory, void* workspace, int32_t* status, void* stream, float* memory_out,
                                             float* grad_blob, float* d_before_highway, float* d_rnn_init)
{
    if (!g || !blob || !tokens || !lengths || !d_memory || !workspace || !status || !memory_out || !grad_blob) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_ENCODER) return twv_fail(TWV_E_INVALID, "the handle was created for the post net");
    if ((before_highway && !d_before_highway) || (rnn_init && !d_rnn_init)) return twv_fail(TWV_E_INVALID, "null argument: before_highway / rnn_init need their d_ outputs");
    GRAD_CHK(twv_tacotron_encoder_grad_forward(g, blob, tokens, lengths, before_highway, rnn_init, mask1, mask2, workspace, status, stream, memory_out));
    return twv_tacotron_encoder_grad_backward(g, blob, tokens, lengths, d_memory, workspace, status, stream, grad_blob, d_before_highway, d_rnn_init);
}

extern "C" int twv_tacotron_postnet_grad_forward(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, void* workspace, int32_t* status,
                                                 void* stream, float* linear_out)
{
    if (!g || !blob || !mel || !workspace || !status || !linear_out) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_POST) return twv_fail(TWV_E_INVALID, "the handle was created for the encoder");
    CgRun r;
    GRAD_CHK(cg_begin(g, r, blob, workspace, status, stream, nullptr));
    const TacoCbhgBlob& w = g->w;
    const CgCarve& c = r.c;
    const int F = g->F;
    GRAD_CHK(r.g->mark(0));
    GRAD_CHK(cbhg_forward(r, mel, nullptr, nullptr, nullptr));
    {
        RowsArgs a = r.rows_args(c.out, 2 * kU, 2 * kU, 1, 0, blob + w.lW, F, F, blob + w.lb);
        a.C = linear_out; a.ldc = F;
        r.launch(a);
    }
    GRAD_HIPCHK(hipGetLastError());
    g->forwarded = 1; g->has_bh = 0; g->has_init = 0;
    return TWV_OK;
}

// (mel: the forward's input once more -- the bank's kernel gradients are products with it)
extern "C" int twv_tacotron_postnet_grad_backward(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, const float* d_linear, void* workspace,
                                                  int32_t* status, void* stream, float* grad_blob, float* d_mel)
{
    if (!g || !blob || !mel || !d_linear || !workspace || !status || !grad_blob || !d_mel) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_POST) return twv_fail(TWV_E_INVALID, "the handle was created for the encoder");
    if (!g->forwarded) return twv_fail(TWV_E_INVALID, "backward: no forward has been made on this handle (twv_tacotron_postnet_grad_forward)");
    CgRun r;
    GRAD_CHK(cg_begin(g, r, blob, workspace, status, stream, grad_blob));
    const TacoCbhgBlob& w = g->w;
    const CgCarve& c = r.c;
    const int F = g->F, M = w.Cin, rows = r.rows;
    GRAD_CHK(r.g->mark(1));
    r.data_grad(d_linear, F, F, blob + w.lW, F, 2 * kU, 1, c.dOut, 2 * kU, 0);
    GRAD_CHK(cbhg_backward_data(r, nullptr, nullptr, nullptr));
    GRAD_HIPCHK(hipMemcpyAsync(d_mel, c.dX, (size_t)rows * M * 4, hipMemcpyDeviceToDevice, r.st));
    GRAD_CHK(r.g->mark(3));
    GRAD_CHK(cbhg_weight_grads(r, mel));
    GRAD_CHK(r.g->wgrad(c.out, 2 * kU, 2 * kU, d_linear, F, F, w.lW, rows)); r.colsum(d_linear, F, F, w.lb);
    GRAD_HIPCHK(hipGetLastError());
    GRAD_CHK(r.g->mark(4));
    return TWV_OK;
}

extern "C" int twv_tacotron_postnet_grad_run(twv_tacotron_cbhg_grad* g, const float* blob, const float* mel, const float* d_linear, void* workspace,
                                             int32_t* status, void* stream, float* linear_out, float* grad_blob, float* d_mel)
{
    if (!g || !blob || !mel || !d_linear || !workspace || !status || !linear_out || !grad_blob || !d_mel) return twv_fail(TWV_E_INVALID, "null argument");
    if (g->which != TWV_CBHG_POST) return twv_fail(TWV_E_INVALID, "the handle was created for the encoder");
    GRAD_CHK(twv_tacotron_postnet_grad_forward(g, blob, mel, workspace, status, stream, linear_out));
    return twv_tacotron_postnet_grad_backward(g, blob, mel, d_linear, workspace, status, stream, grad_blob, d_mel);
}

// after a run with timing on: waits for it and gives the milliseconds of (a) the recording forward, (b) the GRUs' backward through time,
// (c) the row-wise backward (pointwise kernels and the dx products), (d) the weight-gradient products
extern "C" int twv_tacotron_cbhg_grad_phase_ms(twv_tacotron_cbhg_grad* g, double* ms4)
{
    if (!g || !ms4) return twv_fail(TWV_E_INVALID, "null argument");
    return g->phase_ms(4, ms4, "twv_tacotron_cbhg_grad_set_timing");
}

extern "C" int twv_tacotron_linear_loss_grad(const float* linear, const float* linear_targets, const float* loss_coeff, int batch, int t_out,
                                             int num_freq, int prioritize_loss, double sample_rate, float* d_linear, void* stream)
{
    if (!linear || !linear_targets || !loss_coeff || !d_linear) return twv_fail(TWV_E_INVALID, "null argument");
    if (batch < 1 || t_out < 1 || num_freq < 1) return twv_fail(TWV_E_INVALID, "batch, t_out and num_freq must be >= 1");
    if (prioritize_loss && !(sample_rate > 0.0)) return twv_fail(TWV_E_INVALID, "prioritize_loss needs sample_rate > 0");
    const long long per = (long long)t_out * num_freq, total = per * batch;
    int lo = 0, hi = 0;
    double w0 = 1.0 / (double)total, w1 = 0.0;
    if (prioritize_loss) {              // tacotron.py:269-272, the band exactly as twv_tacotron_loss computes it
        const int hi_ = (int)(5000 / (sample_rate * 0.5) * num_freq), lo_ = (int)(165 / (sample_rate * 0.5) * num_freq);
        lo = lo_ < 0 ? 0 : (lo_ > num_freq ? num_freq : lo_);
        hi = hi_ < lo ? lo : (hi_ > num_freq ? num_freq : hi_);
        w0 = 0.5 / (double)total;
        w1 = hi > lo ? 0.5 / ((double)batch * t_out * (hi - lo)) : 0.0;
    }
    hipLaunchKernelGGL(cg_linear_loss_grad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, linear, linear_targets, loss_coeff, per,
                       num_freq, lo, hi, (float)w0, (float)w1, total, d_linear);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}
