// twv_audio.hip -- MI355X (gfx950) spectrogram -> waveform path of the reference synthesizer + its C-ABI (include/twv_amd.h).
//
// Replaces, for hccho2/Tacotron-Wavenet-Vocoder-Korean (citations into /root/reference):
//   synthesizer.py:258 audio_out = inv_linear_spectrogram(wav.T, hparams)
//   utils/audio.py:77-92   inv_linear_spectrogram: _denormalize (:222-227) -> _db_to_amp (:205-206) -> ** power -> _griffin_lim -> inv_preemphasis
//   utils/audio.py:127-137 _griffin_lim: random initial phase, griffin_lim_iters x {librosa.stft -> unit phase -> librosa.istft}
//   utils/audio.py:27-30   inv_preemphasis = lfilter([1], [1, -k])
//   utils/audio.py:95-110  inv_mel_spectrogram (the same loop after _mel_to_linear, :187-191) and every _denormalize setting (:222-234)
// The FFTs are plain library transforms (hipFFT, batched over every frame of every utterance); framing, windowing,
// overlap-add with the window sum-of-squares normalisation, reflect padding, phase projection, magnitude shaping and the
// de-emphasis recurrence are hand-written kernels.  The spectrogram stays in Tacotron's own (utterance, frame, bin) layout,
// which is already the batched-FFT layout.  Floating-point work: parity is by tolerance against the float64 numpy restatement.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/twv_amd.h"
#include "twv_dev.hpp"

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

struct twv_griffin_lim {
    int n_fft, hop, win, frames, batch, nbin, len;        // len = hop * (frames - 1) samples per utterance (ragged: of the longest)
    long long tf, ts, tc;                                 // frames, samples and de-emphasis chunks of the whole batch
    hipfftHandle c2r, r2c;
    bool have_plans;
    // twv_griffin_lim_create_ragged only: the table the ragged kernels read, three arrays of batch + 1 ascending offsets -- frames,
    // samples, de-emphasis chunks -- so utterance b has f0[b+1] - f0[b] frames, s0[b+1] - s0[b] samples, c0[b+1] - c0[b] chunks
    bool ragged;
    std::vector<long long> table;
};

#define GA_STRIDE(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)
static inline int ga_grid(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g)); }

// periodic Hann of win samples, zero-padded symmetrically to n_fft  [librosa.filters.get_window + util.pad_center]
__device__ __forceinline__ float ga_window(int k, int n_fft, int win)
{
    const int j = k - (n_fft - win) / 2;
    if (j < 0 || j >= win) return 0.0f;
    return 0.5f - 0.5f * cospif(2.0f * (float)j / (float)win);
}
// utils/audio.py:222-234 _denormalize.  mode: 0 none, 1 clip + symmetric, 2 clip + asymmetric, 3 symmetric, 4 asymmetric
__device__ __forceinline__ float ga_denorm(float x, int mode, float max_abs, float min_db)
{
    if (mode == 0) return x;
    if (mode == 1) x = x < -max_abs ? -max_abs : (x > max_abs ? max_abs : x);
    if (mode == 2) x = x < 0.0f ? 0.0f : (x > max_abs ? max_abs : x);
    if (mode == 1 || mode == 3) return ((x + max_abs) * -min_db / (2.0f * max_abs)) + min_db;
    return (x * -min_db / max_abs) + min_db;
}
// _denormalize + :205-206 _db_to_amp + "** power": magnitude the Griffin-Lim iterations keep fixed
__global__ void ga_mag_kernel(const float* lin, float* mag, long long n, int mode, float max_abs, float min_db, float ref_db, float power)
{
    GA_STRIDE(i, n) {
        const float db = ga_denorm(lin[i], mode, max_abs, min_db);
        const float s = powf(10.0f, (db + ref_db) * 0.05f);
        mag[i] = powf(s, power);
    }
}
// utils/audio.py:95-110 with :187-191 _mel_to_linear: mag = max(1e-10, inv_basis @ db_to_amp(denormalize(mel) + ref)) ** power.
// One workgroup per frame: the frame's n_mels amplitudes in LDS, one dot product per bin (inv_basis row-major (nbin, n_mels)).
__global__ void ga_mel_mag_kernel(const float* mel, const float* inv_basis, float* mag, int n_mels, int nbin, int mode, float max_abs,
                                  float min_db, float ref_db, float power)
{
    extern __shared__ float ga_amp[];
    const long long row = blockIdx.x;
    for (int m = threadIdx.x; m < n_mels; m += blockDim.x)
        ga_amp[m] = powf(10.0f, (ga_denorm(mel[row * n_mels + m], mode, max_abs, min_db) + ref_db) * 0.05f);
    __syncthreads();
    for (int f = threadIdx.x; f < nbin; f += blockDim.x) {
        const float* w = inv_basis + (long long)f * n_mels;
        float acc = 0.0f;
        for (int m = 0; m < n_mels; ++m) acc += w[m] * ga_amp[m];
        mag[row * nbin + f] = powf(acc > 1e-10f ? acc : 1e-10f, power);
    }
}
// angles = exp(2j*pi*rand) (utils/audio.py:131): spec = mag * angles
__global__ void ga_phase_init_kernel(const float* mag, const float* u, float2* spec, long long n)
{
    GA_STRIDE(i, n) {
        float s, c;
        sincospif(2.0f * u[i], &s, &c);
        spec[i] = make_float2(mag[i] * c, mag[i] * s);
    }
}
// angles = exp(1j * angle(D)) (utils/audio.py:135): spec = mag * D / |D|   (angle(0) = 0)
__global__ void ga_phase_kernel(const float* mag, const float2* D, float2* spec, long long n)
{
    GA_STRIDE(i, n) {
        const float2 d = D[i];
        const float a = hypotf(d.x, d.y);
        const float m = mag[i];
        spec[i] = a > 0.0f ? make_float2(m * (d.x / a), m * (d.y / a)) : make_float2(m, 0.0f);
    }
}
// librosa.istft after the inverse FFTs: y[n] = sum_i w[k] * frame_i[k] / sum_i w[k]^2, k = n + n_fft/2 - i*hop  (already trimmed)
__global__ void ga_ola_kernel(const float* ft, float* y, int batch, int frames, int n_fft, int hop, int win, int len)
{
    const long long total = (long long)batch * len;
    const float inv_n = 1.0f / (float)n_fft;               // hipFFT's C2R is unnormalised, numpy's irfft divides by n
    GA_STRIDE(idx, total) {
        const int b = (int)(idx / len), n = (int)(idx - (long long)b * len);
        const int np_ = n + n_fft / 2;
        int i0 = (np_ - n_fft + hop) / hop; if (np_ - n_fft + 1 <= 0) i0 = 0;      // ceil((np - n_fft + 1) / hop) for positives
        int i1 = np_ / hop; if (i1 > frames - 1) i1 = frames - 1;
        float acc = 0.0f, wss = 0.0f;
        for (int i = i0; i <= i1; ++i) {
            const int k = np_ - i * hop;
            if (k < 0 || k >= n_fft) continue;
            const float w = ga_window(k, n_fft, win);
            acc += w * (ft[((long long)b * frames + i) * n_fft + k] * inv_n);
            wss += w * w;
        }
        y[idx] = wss > 1.17549435e-38f ? acc / wss : acc;
    }
}
// librosa.stft before the forward FFTs: frame_i[k] = w[k] * reflect_pad(y)[i*hop + k]
__global__ void ga_frame_kernel(const float* y, float* fr, int batch, int frames, int n_fft, int hop, int win, int len)
{
    const long long total = (long long)batch * frames * n_fft;
    GA_STRIDE(idx, total) {
        const int k = (int)(idx % n_fft);
        const long long bi = idx / n_fft;
        const int i = (int)(bi % frames), b = (int)(bi / frames);
        const float w = ga_window(k, n_fft, win);
        float v = 0.0f;
        if (w != 0.0f) {
            int j = i * hop + k - n_fft / 2;
            if (j < 0) j = -j;
            if (j >= len) j = 2 * (len - 1) - j;
            v = w * y[(long long)b * len + j];
        }
        fr[idx] = v;
    }
}
// utils/audio.py:27-30 lfilter([1], [1, -k]): y[n] = x[n] + k*y[n-1], exact for the k it is given (any |k| <= 1; the fronts refuse the
// rest).  One thread per 2048-sample chunk, the state carried from chunk to chunk: ga_deemph_ends_kernel leaves each chunk's
// zero-state end value; ga_deemph_kernel chains the ends of the chunks before its own (end_c = local_c + k^2048 * end_{c-1}, every
// chunk before the last is full; at most ~150 steps for 300 k samples) into y[n0 - 1] and runs the recurrence on from there.
// (A zero-state warm-up of any fixed length m leaves k^m of the state out -- after 1024 samples 3e-14 at k = 0.97 but 0.36 at
// 0.999 -- hence the carried state.)
#define GA_DEEMPH_CHUNK 2048
__global__ void ga_deemph_ends_kernel(const float* x, float* ends, int batch, int len, float k)
{
    const int nchunk = (len + GA_DEEMPH_CHUNK - 1) / GA_DEEMPH_CHUNK;
    const long long total = (long long)batch * nchunk;
    GA_STRIDE(idx, total) {
        const int b = (int)(idx / nchunk), c = (int)(idx - (long long)b * nchunk);
        const float* xs = x + (long long)b * len;
        const int n0 = c * GA_DEEMPH_CHUNK, n1 = n0 + GA_DEEMPH_CHUNK < len ? n0 + GA_DEEMPH_CHUNK : len;
        float acc = 0.0f;
        for (int n = n0; n < n1; ++n) acc = xs[n] + k * acc;
        ends[idx] = acc;
    }
}
__global__ void ga_deemph_kernel(const float* x, const float* ends, float* y, int batch, int len, float k, float k_chunk)
{
    const int nchunk = (len + GA_DEEMPH_CHUNK - 1) / GA_DEEMPH_CHUNK;
    const long long total = (long long)batch * nchunk;
    GA_STRIDE(idx, total) {
        const int b = (int)(idx / nchunk), c = (int)(idx - (long long)b * nchunk);
        const float* xs = x + (long long)b * len;
        const float* es = ends + (long long)b * nchunk;
        float* ys = y + (long long)b * len;
        const int n0 = c * GA_DEEMPH_CHUNK, n1 = n0 + GA_DEEMPH_CHUNK < len ? n0 + GA_DEEMPH_CHUNK : len;
        float acc = 0.0f;
        for (int j = 0; j < c; ++j) acc = es[j] + k_chunk * acc;          // = y[n0 - 1]
        for (int n = n0; n < n1; ++n) { acc = xs[n] + k * acc; ys[n] = acc; }
    }
}
// ---- utterances of unequal lengths (twv_griffin_lim_create_ragged): the four kernels above with per-utterance boundaries ----
// The flat index runs over the packed batch; which utterance an element belongs to comes from the handle's offset table (off:
// nb + 1 ascending 64-bit entries, off[0] = 0, no empty utterance).  Every workgroup searches the table for its first and its last
// element -- the same values in every lane, so scalar work -- and only a workgroup that straddles a boundary searches per lane,
// between those two.  Workgroups of 256, 64-bit indices.
// largest b in [lo, hi] with off[b] <= x  (off[lo] <= x)
__device__ __forceinline__ int ga_utt_of(const long long* __restrict__ off, int lo, int hi, long long x)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// A workgroup takes tiles of `tile` consecutive elements, one table search per tile: the search is a chain of dependent loads, which
// a tile of 256 elements does not cover (measured: DESIGN.md section 3g).  At most GA_RAGGED_BLOCKS workgroups, grid-stride beyond.
#define GA_RAGGED_TILE 2048
#define GA_RAGGED_BLOCKS 2048
#define GA_RAGGED_STRIDE(base, n, tile) for (long long base = (long long)blockIdx.x * (tile); base < (n); base += (long long)gridDim.x * (tile))
static inline int ga_ragged_grid(long long n, int tile) { long long g = (n + tile - 1) / tile; return (int)(g < 1 ? 1 : (g > GA_RAGGED_BLOCKS ? GA_RAGGED_BLOCKS : g)); }

// ga_ola_kernel's arithmetic and term order; the contributing frames are clipped to utterance b's own [0, frames_b - 1]
__global__ void ga_ola_ragged_kernel(const float* ft, float* y, const long long* __restrict__ f0, const long long* __restrict__ s0, int nb,
                                     long long total, int n_fft, int hop, int win)
{
    const float inv_n = 1.0f / (float)n_fft;
    GA_RAGGED_STRIDE(base, total, GA_RAGGED_TILE) {
        const long long last = base + GA_RAGGED_TILE - 1 < total ? base + GA_RAGGED_TILE - 1 : total - 1;
        const int blo = ga_utt_of(s0, 0, nb - 1, base), bhi = ga_utt_of(s0, 0, nb - 1, last);     // two independent chains of loads
        for (long long idx = base + threadIdx.x; idx <= last; idx += 256) {
            const int b = blo == bhi ? blo : ga_utt_of(s0, blo, bhi, idx);
            const long long fb = f0[b];
            const int frames = (int)(f0[b + 1] - fb), n = (int)(idx - s0[b]);
            const int np_ = n + n_fft / 2;
            int i0 = (np_ - n_fft + hop) / hop; if (np_ - n_fft + 1 <= 0) i0 = 0;
            int i1 = np_ / hop; if (i1 > frames - 1) i1 = frames - 1;
            float acc = 0.0f, wss = 0.0f;
            for (int i = i0; i <= i1; ++i) {
                const int k = np_ - i * hop;
                if (k < 0 || k >= n_fft) continue;
                const float w = ga_window(k, n_fft, win);
                acc += w * (ft[(fb + i) * n_fft + k] * inv_n);
                wss += w * w;
            }
            y[idx] = wss > 1.17549435e-38f ? acc / wss : acc;
        }
    }
}
// ga_frame_kernel's arithmetic; the reflection is at utterance b's own ends, so no neighbour's sample is read.  The table is
// searched by frame row (idx / n_fft).
__global__ void ga_frame_ragged_kernel(const float* y, float* fr, const long long* __restrict__ f0, const long long* __restrict__ s0, int nb,
                                       long long total, int n_fft, int hop, int win)
{
    GA_RAGGED_STRIDE(base, total, GA_RAGGED_TILE) {
        const long long last = base + GA_RAGGED_TILE - 1 < total ? base + GA_RAGGED_TILE - 1 : total - 1;
        const int blo = ga_utt_of(f0, 0, nb - 1, base / n_fft), bhi = ga_utt_of(f0, 0, nb - 1, last / n_fft);
        for (long long idx = base + threadIdx.x; idx <= last; idx += 256) {
            const int k = (int)(idx % n_fft);
            const long long row = idx / n_fft;
            const int b = blo == bhi ? blo : ga_utt_of(f0, blo, bhi, row);
            const long long sb = s0[b];
            const int i = (int)(row - f0[b]), len = (int)(s0[b + 1] - sb);
            const float w = ga_window(k, n_fft, win);
            float v = 0.0f;
            if (w != 0.0f) {
                int j = i * hop + k - n_fft / 2;
                if (j < 0) j = -j;
                if (j >= len) j = 2 * (len - 1) - j;
                v = w * y[sb + j];
            }
            fr[idx] = v;
        }
    }
}
// ga_deemph_ends_kernel / ga_deemph_kernel over the packed chunks: utterance b has c0[b+1] - c0[b] = ceil(len_b / 2048) of them and
// the chain of chunk ends restarts from a zero state at c0[b]; an utterance of one chunk reads no `ends` entry
__global__ void ga_deemph_ends_ragged_kernel(const float* x, float* ends, const long long* __restrict__ s0, const long long* __restrict__ c0,
                                             int nb, long long total, float k)
{
    GA_RAGGED_STRIDE(base, total, 256) {                   // one chunk of 2048 samples per lane
        const long long idx = base + threadIdx.x, last = base + 255 < total ? base + 255 : total - 1;
        const int blo = ga_utt_of(c0, 0, nb - 1, base), bhi = ga_utt_of(c0, 0, nb - 1, last);
        if (idx >= total) continue;
        const int b = blo == bhi ? blo : ga_utt_of(c0, blo, bhi, idx);
        const int c = (int)(idx - c0[b]), len = (int)(s0[b + 1] - s0[b]);
        const float* xs = x + s0[b];
        const int n0 = c * GA_DEEMPH_CHUNK, n1 = n0 + GA_DEEMPH_CHUNK < len ? n0 + GA_DEEMPH_CHUNK : len;
        float acc = 0.0f;
        for (int n = n0; n < n1; ++n) acc = xs[n] + k * acc;
        ends[idx] = acc;
    }
}
__global__ void ga_deemph_ragged_kernel(const float* x, const float* ends, float* y, const long long* __restrict__ s0,
                                        const long long* __restrict__ c0, int nb, long long total, float k, float k_chunk)
{
    GA_RAGGED_STRIDE(base, total, 256) {                   // one chunk of 2048 samples per lane
        const long long idx = base + threadIdx.x, last = base + 255 < total ? base + 255 : total - 1;
        const int blo = ga_utt_of(c0, 0, nb - 1, base), bhi = ga_utt_of(c0, 0, nb - 1, last);
        if (idx >= total) continue;
        const int b = blo == bhi ? blo : ga_utt_of(c0, blo, bhi, idx);
        const int c = (int)(idx - c0[b]), len = (int)(s0[b + 1] - s0[b]);
        const float* xs = x + s0[b];
        const float* es = ends + c0[b];
        float* ys = y + s0[b];
        const int n0 = c * GA_DEEMPH_CHUNK, n1 = n0 + GA_DEEMPH_CHUNK < len ? n0 + GA_DEEMPH_CHUNK : len;
        float acc = 0.0f;
        for (int j = 0; j < c; ++j) acc = es[j] + k_chunk * acc;          // = y[n0 - 1] of this utterance
        for (int n = n0; n < n1; ++n) { acc = xs[n] + k * acc; ys[n] = acc; }
    }
}
static bool ga_preemphasis_ok(double k) { return k >= -1.0 && k <= 1.0; }      // false for NaN

static long long ga_chunks(long long len) { return (len + GA_DEEMPH_CHUNK - 1) / GA_DEEMPH_CHUNK; }

extern "C" int twv_griffin_lim_create(int n_fft, int hop, int win_length, int n_frames, int batch, twv_griffin_lim** out)
{
    if (!out || n_fft < 8 || (n_fft & 1) || hop < 1 || win_length < 1 || win_length > n_fft || n_frames < 2 || batch < 1)
        return twv_fail(TWV_E_INVALID, "bad argument");
    if ((long long)hop * (n_frames - 1) <= n_fft / 2) return twv_fail(TWV_E_INVALID, "signal shorter than the reflect padding (n_fft/2)");
    twv_griffin_lim* h = new twv_griffin_lim();
    h->n_fft = n_fft; h->hop = hop; h->win = win_length; h->frames = n_frames; h->batch = batch; h->nbin = n_fft / 2 + 1;
    h->len = hop * (n_frames - 1);
    h->tf = (long long)batch * n_frames; h->ts = (long long)batch * h->len; h->tc = batch * ga_chunks(h->len);
    h->have_plans = false;
    h->ragged = false;
    *out = h;
    return TWV_OK;
}
extern "C" int twv_griffin_lim_create_ragged(int n_fft, int hop, int win_length, const int32_t* n_frames_host, int batch, twv_griffin_lim** out)
{
    if (!out || n_fft < 8 || (n_fft & 1) || hop < 1 || win_length < 1 || win_length > n_fft || !n_frames_host || batch < 1)
        return twv_fail(TWV_E_INVALID, "bad argument");
    std::vector<long long> table(3 * ((size_t)batch + 1), 0);
    long long* f0 = table.data(); long long* s0 = f0 + batch + 1; long long* c0 = s0 + batch + 1;
    int longest = 0;
    for (int b = 0; b < batch; ++b) {
        const int T = n_frames_host[b];
        if (T < 2) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + ": fewer than 2 frames");
        const long long len = (long long)hop * (T - 1);
        if (len <= n_fft / 2)
            return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + ": signal shorter than the reflect padding (n_fft/2)");
        if (len > 0x7fffffffLL - n_fft) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + ": too many samples");
        f0[b + 1] = f0[b] + T; s0[b + 1] = s0[b] + len; c0[b + 1] = c0[b] + ga_chunks(len);
        if ((int)len > longest) longest = (int)len;
    }
    if (f0[batch] > 0x7fffffffLL) return twv_fail(TWV_E_INVALID, "more frames in the batch than one hipFFT plan takes (2^31 - 1)");
    twv_griffin_lim* h = new twv_griffin_lim();
    h->n_fft = n_fft; h->hop = hop; h->win = win_length; h->frames = 0; h->batch = batch; h->nbin = n_fft / 2 + 1;
    h->len = longest;
    h->tf = f0[batch]; h->ts = s0[batch]; h->tc = c0[batch];
    h->have_plans = false;
    h->ragged = true;
    h->table.swap(table);
    *out = h;
    return TWV_OK;
}
extern "C" void twv_griffin_lim_destroy(twv_griffin_lim* h)
{
    if (h && h->have_plans) { hipfftDestroy(h->c2r); hipfftDestroy(h->r2c); }
    delete h;
}
extern "C" int twv_griffin_lim_samples(const twv_griffin_lim* h) { return h->len; }
extern "C" int64_t twv_griffin_lim_total_frames(const twv_griffin_lim* h) { return h->tf; }
extern "C" int64_t twv_griffin_lim_total_samples(const twv_griffin_lim* h) { return h->ts; }
extern "C" int twv_griffin_lim_offsets(const twv_griffin_lim* h, int64_t* frame_offsets_host, int64_t* sample_offsets_host)
{
    if (!h) return twv_fail(TWV_E_INVALID, "bad argument");
    for (int b = 0; b <= h->batch; ++b) {
        if (frame_offsets_host) frame_offsets_host[b] = h->ragged ? h->table[b] : (long long)b * h->frames;
        if (sample_offsets_host) sample_offsets_host[b] = h->ragged ? h->table[(size_t)h->batch + 1 + b] : (long long)b * h->len;
    }
    return TWV_OK;
}
static size_t ga_table_bytes(const twv_griffin_lim* h) { return h->ragged ? h->table.size() * sizeof(long long) + 256 : 0; }
extern "C" size_t twv_griffin_lim_workspace_bytes(const twv_griffin_lim* h)
{
    return (size_t)(h->tf * h->nbin * 4 + h->tf * h->nbin * 8 * 2 + h->tf * h->n_fft * 4 + h->ts * 4 + h->tc * 4 + 4096) + ga_table_bytes(h);
}

// utils/audio.py:127-137 + :27-30 for magnitudes already in the workspace (ga_workspace): random initial phase, iters x {stft -> unit
// phase -> istft}, inverse pre-emphasis.  Shared by both fronts below.
struct ga_workspace { float* mag; float2* spec; float2* D; float* ft; float* y; float* ends; long long* table; };
static ga_workspace ga_carve(const twv_griffin_lim* h, void* workspace)
{
    const long long bf = h->tf, nspec = bf * h->nbin;
    ga_workspace p;
    char* w = (char*)workspace;
    p.mag = (float*)w; w += (nspec * 4 + 255) / 256 * 256;
    p.spec = (float2*)w; w += (nspec * 8 + 255) / 256 * 256;
    p.D = (float2*)w; w += (nspec * 8 + 255) / 256 * 256;
    p.ft = (float*)w; w += (bf * h->n_fft * 4 + 255) / 256 * 256;
    p.y = (float*)w; w += (h->ts * 4 + 255) / 256 * 256;
    p.ends = (float*)w; w += (h->tc * 4 + 255) / 256 * 256;   // one chunk end of the de-emphasis per 2048 samples of every utterance
    p.table = (long long*)w;                               // ragged handles: the offset table (ga_table_bytes)
    return p;
}
static int ga_griffin_lim_ragged(twv_griffin_lim* h, const ga_workspace& p, const float* uniforms, int iters, double preemphasis, float* out,
                                 hipStream_t st);
static int ga_griffin_lim(twv_griffin_lim* h, const ga_workspace& p, const float* uniforms, int iters, double preemphasis, float* out, hipStream_t st)
{
    if (h->ragged) return ga_griffin_lim_ragged(h, p, uniforms, iters, preemphasis, out, st);
    const long long bf = h->tf, nspec = bf * h->nbin;
    float* mag = p.mag; float2* spec = p.spec; float2* D = p.D; float* ft = p.ft; float* y = p.y;
    if (!h->have_plans) {
        int n[1] = {h->n_fft};
        FFTCHK(hipfftPlanMany(&h->c2r, 1, n, nullptr, 1, h->nbin, nullptr, 1, h->n_fft, HIPFFT_C2R, (int)bf));
        FFTCHK(hipfftPlanMany(&h->r2c, 1, n, nullptr, 1, h->n_fft, nullptr, 1, h->nbin, HIPFFT_R2C, (int)bf));
        h->have_plans = true;
    }
    FFTCHK(hipfftSetStream(h->c2r, st));
    FFTCHK(hipfftSetStream(h->r2c, st));
    hipLaunchKernelGGL(ga_phase_init_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, mag, uniforms, spec, nspec);
    for (int it = 0; it <= iters; ++it) {
        // librosa.istft: inverse FFT of every frame (the C2R transform may overwrite its input: spec is rebuilt each round), overlap-add
        FFTCHK(hipfftExecC2R(h->c2r, (hipfftComplex*)spec, ft));
        hipLaunchKernelGGL(ga_ola_kernel, dim3(ga_grid((long long)h->batch * h->len)), dim3(256), 0, st, ft, y, h->batch, h->frames, h->n_fft, h->hop,
                           h->win, h->len);
        if (it == iters) break;
        // librosa.stft: reflect-padded windowed frames, forward FFT, keep only the phase
        hipLaunchKernelGGL(ga_frame_kernel, dim3(ga_grid(bf * h->n_fft)), dim3(256), 0, st, y, ft, h->batch, h->frames, h->n_fft, h->hop, h->win, h->len);
        FFTCHK(hipfftExecR2C(h->r2c, ft, (hipfftComplex*)D));
        hipLaunchKernelGGL(ga_phase_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, mag, D, spec, nspec);
    }
    const int nchunk = (h->len + GA_DEEMPH_CHUNK - 1) / GA_DEEMPH_CHUNK;
    const dim3 dgrid(ga_grid((long long)h->batch * nchunk));
    if (nchunk > 1)
        hipLaunchKernelGGL(ga_deemph_ends_kernel, dgrid, dim3(256), 0, st, y, p.ends, h->batch, h->len, (float)preemphasis);
    hipLaunchKernelGGL(ga_deemph_kernel, dgrid, dim3(256), 0, st, y, p.ends, out, h->batch, h->len, (float)preemphasis,
                       (float)pow(preemphasis, (double)GA_DEEMPH_CHUNK));
    HIPCHK(hipGetLastError());
    return TWV_OK;
}
// the same sequence for a ragged handle: the per-bin kernels and the plans are flat over the packed frames; overlap-add, framing and
// the de-emphasis read the offset table, which goes into the workspace first, in stream order.  As many launches as above.
static int ga_griffin_lim_ragged(twv_griffin_lim* h, const ga_workspace& p, const float* uniforms, int iters, double preemphasis, float* out,
                                 hipStream_t st)
{
    const long long bf = h->tf, nspec = bf * h->nbin;
    float* mag = p.mag; float2* spec = p.spec; float2* D = p.D; float* ft = p.ft; float* y = p.y;
    const int nb = h->batch;
    const long long* f0 = p.table; const long long* s0 = f0 + nb + 1; const long long* c0 = s0 + nb + 1;
    if (!h->have_plans) {
        int n[1] = {h->n_fft};
        FFTCHK(hipfftPlanMany(&h->c2r, 1, n, nullptr, 1, h->nbin, nullptr, 1, h->n_fft, HIPFFT_C2R, (int)bf));
        FFTCHK(hipfftPlanMany(&h->r2c, 1, n, nullptr, 1, h->n_fft, nullptr, 1, h->nbin, HIPFFT_R2C, (int)bf));
        h->have_plans = true;
    }
    FFTCHK(hipfftSetStream(h->c2r, st));
    FFTCHK(hipfftSetStream(h->r2c, st));
    HIPCHK(hipMemcpyAsync(p.table, h->table.data(), h->table.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ga_phase_init_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, mag, uniforms, spec, nspec);
    for (int it = 0; it <= iters; ++it) {
        FFTCHK(hipfftExecC2R(h->c2r, (hipfftComplex*)spec, ft));
        hipLaunchKernelGGL(ga_ola_ragged_kernel, dim3(ga_ragged_grid(h->ts, GA_RAGGED_TILE)), dim3(256), 0, st, ft, y, f0, s0, nb, h->ts, h->n_fft, h->hop, h->win);
        if (it == iters) break;
        hipLaunchKernelGGL(ga_frame_ragged_kernel, dim3(ga_ragged_grid(bf * h->n_fft, GA_RAGGED_TILE)), dim3(256), 0, st, y, ft, f0, s0, nb, bf * h->n_fft, h->n_fft,
                           h->hop, h->win);
        FFTCHK(hipfftExecR2C(h->r2c, ft, (hipfftComplex*)D));
        hipLaunchKernelGGL(ga_phase_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, mag, D, spec, nspec);
    }
    const dim3 dgrid(ga_ragged_grid(h->tc, 256));
    if (h->tc > nb)                                        // some utterance has more than one chunk
        hipLaunchKernelGGL(ga_deemph_ends_ragged_kernel, dgrid, dim3(256), 0, st, y, p.ends, s0, c0, nb, h->tc, (float)preemphasis);
    hipLaunchKernelGGL(ga_deemph_ragged_kernel, dgrid, dim3(256), 0, st, y, p.ends, out, s0, c0, nb, h->tc, (float)preemphasis,
                       (float)pow(preemphasis, (double)GA_DEEMPH_CHUNK));
    HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_inv_linear_spectrogram(twv_griffin_lim* h, const float* lin, const float* uniforms, int iters, double power, double ref_level_db,
                                          double max_abs_value, double min_level_db, double preemphasis, void* workspace, float* out, void* stream)
{
    if (!ga_preemphasis_ok(preemphasis)) return twv_fail(TWV_E_INVALID, "preemphasis must be in [-1, 1]");
    if (!h || !lin || !uniforms || !workspace || !out || iters < 0) return twv_fail(TWV_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const long long nspec = h->tf * h->nbin;
    const ga_workspace p = ga_carve(h, workspace);
    hipLaunchKernelGGL(ga_mag_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, lin, p.mag, nspec, 1, (float)max_abs_value, (float)min_level_db,
                       (float)ref_level_db, (float)power);
    return ga_griffin_lim(h, p, uniforms, iters, preemphasis, out, st);
}

extern "C" int twv_inv_spectrogram(twv_griffin_lim* h, const float* spec, int n_channels, const float* inv_basis, const float* uniforms,
                                   int iters, double power, double ref_level_db, double max_abs_value, double min_level_db, int norm_mode,
                                   double preemphasis, void* workspace, float* out, void* stream)
{
    if (!ga_preemphasis_ok(preemphasis)) return twv_fail(TWV_E_INVALID, "preemphasis must be in [-1, 1]");
    if (!h || !spec || !uniforms || !workspace || !out || iters < 0 || n_channels < 1 || norm_mode < 0 || norm_mode > 4)
        return twv_fail(TWV_E_INVALID, "bad argument");
    if (!inv_basis && n_channels != h->nbin) return twv_fail(TWV_E_INVALID, "a linear spectrogram has n_fft/2 + 1 channels; a mel spectrogram needs inv_basis");
    if (inv_basis && n_channels > 12288) return twv_fail(TWV_E_INVALID, "n_channels too large");
    hipStream_t st = (hipStream_t)stream;
    const long long bf = h->tf, nspec = bf * h->nbin;
    const ga_workspace p = ga_carve(h, workspace);
    if (inv_basis)
        hipLaunchKernelGGL(ga_mel_mag_kernel, dim3((unsigned)bf), dim3(256), (size_t)n_channels * 4, st, spec, inv_basis, p.mag, n_channels, h->nbin,
                           norm_mode, (float)max_abs_value, (float)min_level_db, (float)ref_level_db, (float)power);
    else
        hipLaunchKernelGGL(ga_mag_kernel, dim3(ga_grid(nspec)), dim3(256), 0, st, spec, p.mag, nspec, norm_mode, (float)max_abs_value,
                           (float)min_level_db, (float)ref_level_db, (float)power);
    return ga_griffin_lim(h, p, uniforms, iters, preemphasis, out, st);
}
