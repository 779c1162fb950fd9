// twv_audio_analysis.hip -- MI355X (gfx950) waveform -> mel / linear spectrogram path + its C-ABI (include/twv_amd.h).
//
// Replaces, for hccho2/Tacotron-Wavenet-Vocoder-Korean (citations into the reference's tree):
//   utils/audio.py:61-75   linearspectrogram / melspectrogram (what datasets/moon.py:113,120 calls per utterance)
//   utils/audio.py:22-25   preemphasis = lfilter([1, -k], [1], wav):  x[0] = wav[0], x[n] = wav[n] - k * wav[n-1]
//   utils/audio.py:139-143 _stft = librosa.stft(n_fft, hop, win): centre=True, reflect padding of n_fft/2, periodic Hann(win) zero-padded
//                          symmetrically to n_fft, 1 + len / hop frames   [librosa's conventions as twv_audio.hip states them]
//   utils/audio.py:181-185 _linear_to_mel = mel_basis @ |D|;  :201-203 _amp_to_db;  :208-220 _normalize
// Three passes for a ragged batch: (1) pre-emphasis + reflect padding + window fused into the FFT input, (2) hipFFT R2C batched over
// every frame of every utterance, (3) ONE read of the complex spectrum that writes both the linear and the mel spectrogram.  The mel
// product is banded: each filter of a mel basis is one short run of bins, so the host keeps (first, count) per filter and the kernel
// makes one dot product per (frame, filter) over magnitudes staged in LDS.  Floating-point work: parity is by tolerance against the
// float64 numpy checker (tests/audio_analysis_ref.py).
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/twv_amd.h"

int twv_fail(int code, const std::string& msg);          // twv_wavenet.hip

#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return twv_fail(TWV_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)
#define FFTCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipfftResult r_ = (expr);                                                                                 \
        if (r_ != HIPFFT_SUCCESS) return twv_fail(TWV_E_HIP, std::string(#expr) + ": hipfft status " + std::to_string((int)r_)); \
    } while (0)

#define SA_TILE 4                 // frames per workgroup of the output kernel (16 KB of magnitudes at n_fft = 2048: eight workgroups per CU)
#define SA_DEEP 4                 // spectrum loads a thread has in flight
#define SA_THREADS 256

struct twv_spectrogram {
    int n_fft, hop, win, n_mels, nbin, max_samples, batch, frames;     // frames = 1 + max_samples / hop (rows per utterance)
    std::vector<float> window;                    // periodic Hann(win), float64 on the host, rounded once
    std::vector<float> band_w;                    // the filters' spans, one after the other
    std::vector<int32_t> band;                    // per filter: first bin, count, offset into band_w
    std::vector<int32_t> lengths;                 // host copy of the last call's lengths (source of the asynchronous upload)
    float* d_window; float* d_band_w; int32_t* d_band;                // device copies, made by the first analyze
    hipfftHandle r2c;
    bool on_device;
};

// one sample of the pre-emphasised, reflect-padded signal (np.pad(lfilter([1, -k], [1], wav), n_fft/2, 'reflect')); s = index into the
// unpadded signal, -n_fft/2 <= s < len + n_fft/2, and len > n_fft/2 makes one reflection enough
__device__ __forceinline__ float sa_sample(const float* wav, int len, int s, float k)
{
    if (s < 0) s = -s;
    if (s >= len) s = 2 * (len - 1) - s;
    const float cur = wav[s];
    return s > 0 ? cur - k * wav[s - 1] : cur;
}

// pass 1: one workgroup per (utterance, frame) row of the FFT input.  Only the win window samples of a row need a product: they are
// formed with consecutive lanes on consecutive samples (coalesced loads of the signal and the window) into LDS; the row is then written
// with VEC floats per store (4 when n_fft % 4 == 0, else 2), zeros outside the window.  Rows past the utterance's last frame: all zeros.
template <int VEC>
__global__ void __launch_bounds__(SA_THREADS) sa_frame_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                              const float* __restrict__ window, float* __restrict__ fr, int frames,
                                                              int n_fft, int hop, int win, int max_samples, float k)
{
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    extern __shared__ float sa_prod[];                   // win products
    const int row = blockIdx.x, b = row / frames, i = row - b * frames;
    const int len = lengths[b];
    const bool live = i < 1 + len / hop;                 // uniform over the workgroup
    vec_t* dst = reinterpret_cast<vec_t*>(fr + (long long)row * n_fft);
    const int lpad = (n_fft - win) / 2;
    if (live) {
        const float* w = wav + (long long)b * max_samples;
        const int s0 = i * hop - n_fft / 2 + lpad;
        for (int j = threadIdx.x; j < win; j += SA_THREADS) sa_prod[j] = window[j] * sa_sample(w, len, s0 + j, k);
    }
    __syncthreads();
    for (int v = threadIdx.x; v < n_fft / VEC; v += SA_THREADS) {
        vec_t o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int j = v * VEC + e - lpad;
            o[e] = (live && j >= 0 && j < win) ? sa_prod[j] : 0.0f;
        }
        dst[v] = o;
    }
}

// utils/audio.py:201-203 + "- ref_level_db" + :208-220.  S is returned through *s_db for the min / max of :216.
__device__ __forceinline__ float sa_normalize(float amp, float min_level, float ref_db, float min_db, float max_abs, int mode, float* s_db)
{
    const float S = 20.0f * log10f(amp > min_level ? amp : min_level) - ref_db;
    *s_db = S;
    if (mode == 0) return S;
    const float t = (S - min_db) / (-min_db);
    float o = (mode == 1 || mode == 3) ? (2.0f * max_abs) * t - max_abs : max_abs * t;
    if (mode == 1) o = o < -max_abs ? -max_abs : (o > max_abs ? max_abs : o);
    if (mode == 2) o = o < 0.0f ? 0.0f : (o > max_abs ? max_abs : o);
    return o;
}

// float min / max through the integer atomics (the bit patterns of non-negative floats order as ints, of negative ones inversely as
// unsigned ints); *addr starts at +inf / -inf
__device__ __forceinline__ void sa_atomic_min(float* addr, float v)
{
    if (v >= 0.0f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void sa_atomic_max(float* addr, float v)
{
    if (v >= 0.0f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__global__ void sa_minmax_init_kernel(float* mm) { mm[0] = INFINITY; mm[1] = -INFINITY; }

// pass 3: SA_TILE consecutive rows per workgroup.  Every bin's magnitude is computed once: written (normalised) to lin_out and kept in LDS;
// then one banded dot product per (row, filter), consecutive threads on consecutive filters of a row so that mel_out is written in runs.
__global__ void __launch_bounds__(SA_THREADS) sa_output_kernel(const float2* __restrict__ D, const int32_t* __restrict__ lengths,
                                                               const float* __restrict__ band_w, const int32_t* __restrict__ band,
                                                               float* __restrict__ mel_out, float* __restrict__ lin_out,
                                                               float* __restrict__ minmax, int rows, int frames, int nbin, int n_mels,
                                                               int hop, float min_level, float ref_db, float min_db, float max_abs, int mode)
{
    extern __shared__ float sa_mag[];                    // SA_TILE x nbin
    const int row0 = blockIdx.x * SA_TILE;
    const int nrow = rows - row0 < SA_TILE ? rows - row0 : SA_TILE;
    float lo = INFINITY, hi = -INFINITY;
    for (int r = 0; r < nrow; ++r) {
        const int row = row0 + r, b = row / frames, i = row - b * frames;
        const bool live = i < 1 + lengths[b] / hop;
        for (int base = threadIdx.x; base < nbin; base += SA_DEEP * SA_THREADS) {
            float2 d[SA_DEEP];
#pragma unroll
            for (int u = 0; u < SA_DEEP; ++u) {            // the loads first: the kernel lives on memory latency
                const int f = base + u * SA_THREADS;
                d[u] = (live && f < nbin) ? D[(long long)row * nbin + f] : make_float2(0.0f, 0.0f);
            }
#pragma unroll
            for (int u = 0; u < SA_DEEP; ++u) {
                const int f = base + u * SA_THREADS;
                if (f >= nbin) break;
                float o = 0.0f, a = 0.0f;
                if (live) {
                    a = sqrtf(d[u].x * d[u].x + d[u].y * d[u].y);
                    if (lin_out) {
                        float S;
                        o = sa_normalize(a, min_level, ref_db, min_db, max_abs, mode, &S);
                        lo = fminf(lo, S); hi = fmaxf(hi, S);
                    }
                }
                sa_mag[r * nbin + f] = a;
                if (lin_out) lin_out[(long long)row * nbin + f] = o;
            }
        }
    }
    __syncthreads();
    if (mel_out) {
        for (int idx = threadIdx.x; idx < nrow * n_mels; idx += SA_THREADS) {
            const int r = idx / n_mels, m = idx - r * n_mels;
            const int row = row0 + r, b = row / frames, i = row - b * frames;
            float o = 0.0f;
            if (i < 1 + lengths[b] / hop) {
                const int first = band[3 * m], count = band[3 * m + 1];
                const float* w = band_w + band[3 * m + 2];
                const float* x = sa_mag + r * nbin + first;
                float acc = 0.0f;
                for (int t = 0; t < count; ++t) acc += w[t] * x[t];
                float S;
                o = sa_normalize(acc, min_level, ref_db, min_db, max_abs, mode, &S);
                lo = fminf(lo, S); hi = fmaxf(hi, S);
            }
            mel_out[(long long)row0 * n_mels + idx] = o;
        }
    }
    if (minmax) {
        for (int off = 32; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if ((threadIdx.x & 63) == 0) {
            if (lo != INFINITY) sa_atomic_min(minmax, lo);
            if (hi != -INFINITY) sa_atomic_max(minmax + 1, hi);
        }
    }
}

extern "C" int twv_spectrogram_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis_host, int max_samples, int batch,
                                      twv_spectrogram** out)
{
    if (!out || n_fft < 8 || (n_fft & 1) || hop < 1 || win_length < 1 || win_length > n_fft || n_mels < 0 || batch < 1)
        return twv_fail(TWV_E_INVALID, "bad argument (n_fft even and >= 8, 1 <= win_length <= n_fft, hop >= 1, batch >= 1)");
    if (n_mels > 0 && !mel_basis_host) return twv_fail(TWV_E_INVALID, "n_mels > 0 needs a mel basis");
    if (max_samples <= n_fft / 2) return twv_fail(TWV_E_INVALID, "signal not longer than the reflect padding (n_fft/2)");
    const long long rows = (long long)batch * (1 + max_samples / hop);
    if (rows > 0x7fffffffLL / SA_TILE) return twv_fail(TWV_E_INVALID, "batch x frames too large");
    twv_spectrogram* h = new twv_spectrogram();
    h->n_fft = n_fft; h->hop = hop; h->win = win_length; h->n_mels = n_mels; h->nbin = n_fft / 2 + 1;
    h->max_samples = max_samples; h->batch = batch; h->frames = 1 + max_samples / hop;
    h->d_window = nullptr; h->d_band_w = nullptr; h->d_band = nullptr; h->on_device = false;
    h->window.resize(win_length);
    for (int j = 0; j < win_length; ++j) h->window[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)win_length));
    h->band.resize(3 * (size_t)n_mels);
    for (int m = 0; m < n_mels; ++m) {
        const float* row = mel_basis_host + (size_t)m * h->nbin;
        int first = 0, last = -1;
        for (int f = 0; f < h->nbin; ++f)
            if (row[f] != 0.0f) { if (last < 0) first = f; last = f; }
        const int count = last < 0 ? 0 : last - first + 1;
        h->band[3 * m] = first; h->band[3 * m + 1] = count; h->band[3 * m + 2] = (int32_t)h->band_w.size();
        h->band_w.insert(h->band_w.end(), row + first, row + first + count);
    }
    *out = h;
    return TWV_OK;
}
extern "C" void twv_spectrogram_destroy(twv_spectrogram* h)
{
    if (!h) return;
    if (h->on_device) {
        hipfftDestroy(h->r2c);
        (void)hipFree(h->d_window); (void)hipFree(h->d_band_w); (void)hipFree(h->d_band);
    }
    delete h;
}
extern "C" int twv_spectrogram_frames(const twv_spectrogram* h) { return h->frames; }

static size_t sa_round(size_t n) { return (n + 255) / 256 * 256; }
extern "C" size_t twv_spectrogram_workspace_bytes(const twv_spectrogram* h)
{
    const size_t rows = (size_t)h->batch * h->frames;
    return sa_round((size_t)h->batch * 4) + sa_round(rows * h->n_fft * 4) + sa_round(rows * h->nbin * 8) + 256;
}

extern "C" int twv_spectrogram_analyze(twv_spectrogram* h, const float* wav, const int32_t* lengths_host, double preemphasis, double ref_level_db,
                                       double min_level_db, double max_abs_value, int norm_mode, void* workspace, float* mel_out, float* lin_out,
                                       float* minmax_out, void* stream)
{
    if (!h || !wav || !workspace || norm_mode < 0 || norm_mode > 4) return twv_fail(TWV_E_INVALID, "bad argument");
    if (mel_out && h->n_mels == 0) return twv_fail(TWV_E_INVALID, "mel_out without a mel basis (n_mels = 0 at create)");
    if (!mel_out && !lin_out) return twv_fail(TWV_E_INVALID, "neither output requested");
    h->lengths.resize(h->batch);
    for (int b = 0; b < h->batch; ++b) {
        const int len = lengths_host ? lengths_host[b] : h->max_samples;
        if (len <= h->n_fft / 2) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + " is not longer than the reflect padding (n_fft/2)");
        if (len > h->max_samples) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + " is longer than max_samples");
        h->lengths[b] = len;
    }
    const size_t lds = (size_t)SA_TILE * h->nbin * 4;
    if (lds > 64 * 1024) return twv_fail(TWV_E_UNSUPPORTED, "n_fft above 8190: the magnitude tile does not fit the LDS budget of the output kernel");
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)h->batch * h->frames;
    if (!h->on_device) {
        HIPCHK(hipMalloc((void**)&h->d_window, h->window.size() * 4));
        HIPCHK(hipMalloc((void**)&h->d_band_w, (h->band_w.size() + 1) * 4));
        HIPCHK(hipMalloc((void**)&h->d_band, (h->band.size() + 1) * 4));
        HIPCHK(hipMemcpy(h->d_window, h->window.data(), h->window.size() * 4, hipMemcpyHostToDevice));
        if (!h->band_w.empty()) HIPCHK(hipMemcpy(h->d_band_w, h->band_w.data(), h->band_w.size() * 4, hipMemcpyHostToDevice));
        if (!h->band.empty()) HIPCHK(hipMemcpy(h->d_band, h->band.data(), h->band.size() * 4, hipMemcpyHostToDevice));
        int n[1] = {h->n_fft};
        FFTCHK(hipfftPlanMany(&h->r2c, 1, n, nullptr, 1, h->n_fft, nullptr, 1, h->nbin, HIPFFT_R2C, (int)rows));
        h->on_device = true;
    }
    FFTCHK(hipfftSetStream(h->r2c, st));
    char* w = (char*)workspace;
    int32_t* d_len = (int32_t*)w; w += sa_round((size_t)h->batch * 4);
    float* fr = (float*)w; w += sa_round((size_t)rows * h->n_fft * 4);
    float2* D = (float2*)w;
    HIPCHK(hipMemcpyAsync(d_len, h->lengths.data(), (size_t)h->batch * 4, hipMemcpyHostToDevice, st));
    if (h->n_fft % 4 == 0)
        hipLaunchKernelGGL(sa_frame_kernel<4>, dim3((unsigned)rows), dim3(SA_THREADS), (size_t)h->win * 4, st, wav, d_len, h->d_window, fr, h->frames, h->n_fft,
                           h->hop, h->win, h->max_samples, (float)preemphasis);
    else
        hipLaunchKernelGGL(sa_frame_kernel<2>, dim3((unsigned)rows), dim3(SA_THREADS), (size_t)h->win * 4, st, wav, d_len, h->d_window, fr, h->frames, h->n_fft,
                           h->hop, h->win, h->max_samples, (float)preemphasis);
    FFTCHK(hipfftExecR2C(h->r2c, fr, (hipfftComplex*)D));
    if (minmax_out) hipLaunchKernelGGL(sa_minmax_init_kernel, dim3(1), dim3(1), 0, st, minmax_out);
    const float min_level = (float)exp(min_level_db / 20.0 * log(10.0));
    hipLaunchKernelGGL(sa_output_kernel, dim3((unsigned)((rows + SA_TILE - 1) / SA_TILE)), dim3(SA_THREADS), lds, st, D, d_len, h->d_band_w, h->d_band,
                       mel_out, lin_out, minmax_out, (int)rows, h->frames, h->nbin, h->n_mels, h->hop, min_level, (float)ref_level_db,
                       (float)min_level_db, (float)max_abs_value, norm_mode);
    HIPCHK(hipGetLastError());
    return TWV_OK;
}
