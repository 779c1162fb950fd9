// What the Tacotron gradient passes share (twv_tacotron_grad.hip: the decoder, twv_tacotron_cbhg_grad.hip: the encoder and the post net;
// DESIGN 3b-g, 3b-h): the check macros, the base of both handles (rocBLAS handle, phase events, the weight-gradient product), the carve's
// `take`, and the row kernel -- every product over rows on a path whose bits must not depend on the batch.
// A kernel defined here is compiled into each file that launches it; its Unit parameter (the file's handle type) gives each copy its own symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_dev.hpp"

#define GRAD_HIPCHK(expr)                                                                                        \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return twv_fail(TWV_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)
#define GRAD_BLASCHK(expr)                                                                                       \
    do {                                                                                                          \
        rocblas_status s_ = (expr);                                                                               \
        if (s_ != rocblas_status_success) return twv_fail(TWV_E_HIP, std::string(#expr) + ": " + rocblas_status_to_string(s_)); \
    } while (0)
// a step that has already reported its failure through twv_fail
#define GRAD_CHK(expr)                                                                                           \
    do {                                                                                                          \
        const int rc_ = (expr);                                                                                   \
        if (rc_ != TWV_OK) return rc_;                                                                            \
    } while (0)

namespace tgrad {

__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
inline int grid_for(long long n) { const long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

// ---- the carve of a workspace or of a workgroup's LDS: consecutive pieces, each rounded up to four floats.  One carve sizes the area
// and places its pieces, for the host and for the kernel.
template <class I>
struct Take {
    I used = 0;
    __host__ __device__ I operator()(I n) { const I o = used; used += (n + 3) & ~(I)3; return o; }
};
struct TakeFloats {             // pieces of a workspace; base null: sizing only
    float* base;
    Take<long long> off;
    float* operator()(long long n) { const long long o = off(n); return base ? base + o : nullptr; }
};

// ---- the row kernel: products over all rows, a convolution of width kw as kw shifted products accumulated in tap order
//   z[r][j] = bias[j] + sum_tap sum_k X[r + tap - left][k] * W[(tap * Cin + k) * ldw + j]        (rows of another utterance read as zeros)
//   act 1: v = max(z, 0) * mask, gate_out = z > 0 ? mask : 0 (mask null = ones; mask and gate_out are (rows, ncols));  act 2: v = sigmoid(z)
//   v *= gate_in;   C = (add ? C : 0) + v;   Y = v * inv[j] + shift[j] (inv null: v) + add1[r][j] + add2[r / T][j]
// float64 accumulators, k ascending, the bias added once in float64 and one rounding: one order of additions per (row, column) whatever
// the number of rows.  grid (rows / kRB, ncols / 256).
constexpr int kRB = 8, kKC = 128, kMaxKw = 16;       // rows a block, K chunk in LDS, widest convolution
struct RowsArgs {
    const float *X, *W, *bias, *mask, *gate_in, *inv, *shift, *add1, *add2;
    float *C, *gate_out, *Y;
    int ldx, ldw, ldc, ldy, ld1, ld2, rows, T, Cin, kw, left, ncols, act, add;
};
template <class Unit>
__global__ void __launch_bounds__(256) grad_rows_kernel(RowsArgs a)
{
    __shared__ double xs[(kRB + kMaxKw) * kKC];       // rows r0 - left .. r0 + kRB - 1 + right of the chunk, then one row of zeros
    __shared__ int idx[kRB * kMaxKw];
    const int tid = threadIdx.x, r0 = blockIdx.x * kRB, nr = min(kRB, a.rows - r0), kw = a.kw, nstage = kRB + kw - 1, zrow = nstage;
    const int j = blockIdx.y * 256 + tid;
    for (int i = tid; i < kRB * kw; i += 256) {
        const int r = i / kw, tap = i - r * kw, row = r0 + r, src = row + tap - a.left;
        const bool ok = r < nr && src >= 0 && src < a.rows && src / a.T == row / a.T;
        idx[r * kMaxKw + tap] = (ok ? r + tap : zrow) * kKC;
    }
    if (tid < kKC) xs[zrow * kKC + tid] = 0.0;
    double acc[kRB];
#pragma unroll
    for (int r = 0; r < kRB; ++r) acc[r] = 0.0;
    for (int k0 = 0; k0 < a.Cin; k0 += kKC) {
        const int kc = min(kKC, a.Cin - k0);
        __syncthreads();
        for (int i = tid; i < nstage * kKC; i += 256) {
            const int s = i / kKC, k = i - s * kKC, src = r0 - a.left + s;
            xs[i] = (src >= 0 && src < a.rows && k < kc) ? (double)a.X[(long long)src * a.ldx + k0 + k] : 0.0;
        }
        __syncthreads();
        if (j < a.ncols) {
            for (int tap = 0; tap < kw; ++tap) {
                int o[kRB];
#pragma unroll
                for (int r = 0; r < kRB; ++r) o[r] = idx[r * kMaxKw + tap];
                const float* wp = a.W + ((long long)tap * a.Cin + k0) * a.ldw + j;
                for (int k = 0; k < kc; ++k) {
                    const double w = (double)wp[(long long)k * a.ldw];
#pragma unroll
                    for (int r = 0; r < kRB; ++r) acc[r] = fma(w, xs[o[r] + k], acc[r]);
                }
            }
        }
    }
    if (j >= a.ncols) return;
#pragma unroll
    for (int r = 0; r < kRB; ++r) {
        if (r >= nr) continue;
        const long long row = r0 + r;
        float v = (float)(acc[r] + (a.bias ? (double)a.bias[j] : 0.0));
        if (a.act == 1) {
            const float m = a.mask ? a.mask[row * a.ncols + j] : 1.0f;
            if (a.gate_out) a.gate_out[row * a.ncols + j] = v > 0.0f ? m : 0.0f;
            v = fmaxf(v, 0.0f) * m;
        } else if (a.act == 2) v = sigmoidf_(v);
        if (a.gate_in) v *= a.gate_in[row * a.ncols + j];
        if (a.C) { const long long o = row * a.ldc + j; a.C[o] = a.add ? a.C[o] + v : v; }
        if (a.Y) {
            float y = a.inv ? v * a.inv[j] + a.shift[j] : v;
            if (a.add1) y = y + a.add1[row * a.ld1 + j];
            if (a.add2) y = y + a.add2[(row / a.T) * a.ld2 + j];
            a.Y[row * a.ldy + j] = y;
        }
    }
}
// the product every caller starts from: rows of T an utterance; the caller sets what it wants of act / mask / gate / C / Y / add
inline RowsArgs rows_args(const float* X, int ldx, int rows, int T, int Cin, int kw, int left, const float* W, int ldw, int ncols, const float* bias)
{
    RowsArgs a;
    memset(&a, 0, sizeof(a));
    a.X = X; a.ldx = ldx; a.Cin = Cin; a.kw = kw; a.left = left; a.W = W; a.ldw = ldw; a.ncols = ncols; a.bias = bias; a.rows = rows; a.T = T;
    return a;
}
template <class Unit>
void launch_rows(hipStream_t st, const RowsArgs& a)
{
    hipLaunchKernelGGL(grad_rows_kernel<Unit>, dim3((a.rows + kRB - 1) / kRB, (a.ncols + 255) / 256), dim3(256), 0, st, a);
}

template <class Unit>
__global__ void grad_mul_kernel(float* x, const float* g, long long total)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) x[i] *= g[i];
}
template <class Unit>
void launch_mul(hipStream_t st, float* x, const float* g, long long total)
{
    hipLaunchKernelGGL(grad_mul_kernel<Unit>, dim3(grid_for(total)), dim3(256), 0, st, x, g, total);
}

// ---- what both handles are: the rocBLAS handle (made by the first run), the route label, the workspace size, the events at the phase
// boundaries of a run with timing on, and the stream and gradient blob of the run in progress
struct Handle {
    static constexpr int kMaxMarks = 5;
    rocblas_handle blas = nullptr;
    std::string route;
    long long ws_floats = 0;
    int timing = 0;                // *_set_timing: events at the phase boundaries of the next runs
    hipEvent_t ev[kMaxMarks] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipStream_t st = nullptr;
    float* grad = nullptr;

    ~Handle()
    {
        if (blas) rocblas_destroy_handle(blas);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    // the start of every run: rocBLAS on the run's stream, status cleared, the whole gradient blob (if the run writes one) zeroed
    int begin(hipStream_t stream, int32_t* status, float* grad_blob, long long blob_floats)
    {
        st = stream; grad = grad_blob;
        if (!blas) {
            GRAD_BLASCHK(rocblas_create_handle(&blas));
            GRAD_BLASCHK(rocblas_set_atomics_mode(blas, rocblas_atomics_not_allowed));     // the same bits on every run
        }
        GRAD_BLASCHK(rocblas_set_stream(blas, st));
        GRAD_BLASCHK(rocblas_set_pointer_mode(blas, rocblas_pointer_mode_host));
        GRAD_HIPCHK(hipMemsetAsync(status, 0, 16, st));
        if (grad_blob) GRAD_HIPCHK(hipMemsetAsync(grad_blob, 0, (size_t)blob_floats * 4, st));
        return TWV_OK;
    }
    int mark(int i)
    {
        if (!timing) return TWV_OK;
        if (!ev[i]) GRAD_HIPCHK(hipEventCreate(&ev[i]));
        GRAD_HIPCHK(hipEventRecord(ev[i], st));
        return TWV_OK;
    }
    int set_timing(int on) { timing = on ? 1 : 0; return TWV_OK; }
    // after a run with timing on: waits for it and gives the milliseconds between marks 0 .. n
    int phase_ms(int n, double* out, const char* set_timing_name)
    {
        if (!ev[n]) return twv_fail(TWV_E_INVALID, std::string("no run with timing on (") + set_timing_name + ") has been made");
        GRAD_HIPCHK(hipEventSynchronize(ev[n]));
        for (int i = 0; i < n; ++i) { float ms = 0.0f; GRAD_HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); out[i] = (double)ms; }
        return TWV_OK;
    }
    // grad[off .. off + K * Nc) = X^T (K x nrows) . D (nrows x Nc): row-major = rocBLAS (Nc x K) = D-as-stored . X^T
    int wgrad(const float* X, int ldx, int K, const float* D, int ldd, int Nc, long long off, long long nrows)
    {
        const float one = 1.0f, zero = 0.0f;
        GRAD_BLASCHK(rocblas_sgemm(blas, rocblas_operation_none, rocblas_operation_transpose, Nc, K, (int)nrows, &one, D, ldd, X, ldx, &zero, grad + off, Nc));
        return TWV_OK;
    }
};

}  // namespace tgrad
