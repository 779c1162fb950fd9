// twv_resample.hip -- MI355X (gfx950) band-limited rational resampler + its C-ABI (include/twv_amd.h).
//
// Replaces, for hccho2/Tacotron-Wavenet-Vocoder-Korean (citations into the reference's tree):
//   utils/audio.py:11-12   load_wav = librosa.core.load(path, sr=sr)[0]: channels averaged, then resampled to sr
//   generate.py:90         the same call for --wav_seed
// The arithmetic is this project's contract ("Resampling"); [RECALLED] resampy's kaiser_best parameters, unpinned:
//   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M);  n_out = ceil(n_in * L / M)
//   y[t] = sum_n x[n] * s * h(s * (t * M / L - n)),  h(u) = r sinc(r u) I0(beta sqrt(1 - (u/Z)^2)) / I0(beta) for |u| < Z, else 0
// With t * M = q * L + p (64-bit integers) the position is q + p / L: L filter phases, no floating-point time.  The host tabulates
//   c[p][k] = s * h(s * (k - W + p / L)),  k = 0 .. 2W - 1,  W = ceil(Z / s) rounded up to a multiple of 4
// in double, rounded once to float32 (the taps the rounding of W adds lie outside |u| < Z and are exactly 0), so that
//   y[t] = sum_k c[p][k] * x[q + W - k].
// Kernel: outputs of one phase recur every L samples, so the lanes of a wave take t = t0 + L * lane: they share the coefficient row
// (a wave-uniform, scalar load) and read x from an LDS-staged span at stride M.  One workgroup = L * R consecutive outputs of one
// utterance (R "rounds"), its R * M + 2W input samples staged once (format conversion and channel average on the way in), results
// gathered in LDS and written in order.  No waits between workgroups, no atomics; a sum's order depends on the tap index alone.
#include <hip/hip_runtime.h>
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

#define RS_THREADS 512
#define RS_WAVES (RS_THREADS / 64)
#define RS_ZEROS 64                            // zero crossings of the window on either side            [RECALLED] kaiser_best
#define RS_ROLLOFF 0.9475937167399596          //                                                        [RECALLED]
#define RS_BETA 14.769656459379492             //                                                        [RECALLED]
#define RS_TABLE_CAP (1u << 20)                // floats of L x taps: 4 MiB, one XCD's L2
#define RS_LDS_CAP (80 * 1024)                 // bytes of LDS a workgroup may take: two workgroups per CU
#define RS_LDS_GROW (64 * 1024)                // rounds are doubled towards RS_TILE_OUT outputs while the tile stays below this
#define RS_TILE_OUT 4096

struct twv_resampler {
    int sr_in, sr_out, L, M, W, taps, max_in, batch, out_stride;
    int lr, chunks;                            // lanes of a wave that take rounds (64, 16 or 4); rounds per workgroup = lr * chunks
    size_t lds_bytes;
    std::vector<float> table;                  // L x taps
    std::vector<int32_t> lengths;              // per utterance: n_in, n_out (source of the asynchronous upload)
    const void* table_at;                      // the workspace that holds the table
    std::string name;
};

// the gathered outputs of a tile sit at o + o / 32: lanes that store at stride L (a multiple of 32 at L = 160) spread over the banks
__host__ __device__ __forceinline__ int rs_ys(int o) { return o + (o >> 5); }

static size_t rs_lds_floats(int L, int M, int taps, int rounds) { return (size_t)rounds * M + taps + rs_ys(L * rounds) + 1; }

template <int LR>
__global__ void __launch_bounds__(RS_THREADS) rs_resample_kernel(const void* __restrict__ in, int fmt, int channels,
                                                                 const int32_t* __restrict__ lens, const float* __restrict__ ctab,
                                                                 float* __restrict__ out, int L, int M, int taps, int chunks, int max_in,
                                                                 int out_stride, int tiles)
{
    extern __shared__ float rs_lds[];
    const int R = LR * chunks, span = R * M + taps, tile_out = L * R;
    float* xs = rs_lds;                                  // x[base + i], base = tile * R * M - W
    float* ys = rs_lds + span;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int len = lens[2 * b], n_out = lens[2 * b + 1];
    const long long T0 = (long long)tile * tile_out;
    float* orow = out + (long long)b * out_stride;
    if (T0 >= n_out) {                                   // uniform over the workgroup: a tile past the utterance's end is zeros
        for (int o = threadIdx.x; o < tile_out && T0 + o < out_stride; o += RS_THREADS) orow[T0 + o] = 0.0f;
        return;
    }
    const long long base = (long long)tile * R * M - taps / 2;
    const long long row0 = (long long)b * max_in;
    for (int i = threadIdx.x; i < span; i += RS_THREADS) {
        const long long gi = base + i;
        float v = 0.0f;
        if (gi >= 0 && gi < len) {
            if (fmt == 0) {
                if (channels == 1) v = static_cast<const float*>(in)[row0 + gi];
                else { const float2 f = static_cast<const float2*>(in)[row0 + gi]; v = (f.x + f.y) * 0.5f; }
            } else {
                if (channels == 1) v = (float)static_cast<const short*>(in)[row0 + gi] * (1.0f / 32768.0f);
                else { const short2 f = static_cast<const short2*>(in)[row0 + gi]; v = (float)((int)f.x + (int)f.y) * (0.5f / 32768.0f); }
            }
        }
        xs[i] = v;
    }
    __syncthreads();
    constexpr int G = 64 / LR;                           // phases a wave has in flight
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int items = ((L + G - 1) / G) * chunks;
    for (int item = wave; item < items; item += RS_WAVES) {
        const int pg = item / chunks, c = item - pg * chunks;
        int p = pg * G + lane / LR;
        const bool live = p < L;
        if (!live) p = L - 1;
        const int r = lane % LR + LR * c;
        const int pm = p * M;
        int q0 = pm / L, row = pm - q0 * L;              // t * M = (T0 + p + L r) M: q = tile R M + r M + q0, phase = row
        if (LR == 64) { q0 = __builtin_amdgcn_readfirstlane(q0); row = __builtin_amdgcn_readfirstlane(row); }
        const float* cr = ctab + (size_t)row * taps;
        const float* xp = xs + r * M + q0 + taps;        // x[q + W - k] = xp[-k]
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 4
        for (int k = 0; k < taps; k += 4) {
            const float4 cv = *reinterpret_cast<const float4*>(cr + k);
            a0 = __builtin_fmaf(cv.x, xp[-k], a0);
            a1 = __builtin_fmaf(cv.y, xp[-k - 1], a1);
            a2 = __builtin_fmaf(cv.z, xp[-k - 2], a2);
            a3 = __builtin_fmaf(cv.w, xp[-k - 3], a3);
        }
        if (live) ys[rs_ys(p + L * r)] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < tile_out && T0 + o < out_stride; o += RS_THREADS) orow[T0 + o] = T0 + o < n_out ? ys[rs_ys(o)] : 0.0f;
}

// I0 by its power series, sum ((x/2)^k / k!)^2: every term positive, 45 terms at x = 14.8
static double rs_i0(double x)
{
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        const double f = x / (2.0 * k);
        term *= f * f;
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static long long rs_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

static long long rs_out_samples(const twv_resampler* h, long long n_in) { return (n_in * h->L + h->M - 1) / h->M; }

extern "C" int twv_resample_create(int sr_in, int sr_out, int max_samples_in, int batch, twv_resampler** out)
{
    if (!out || sr_in <= 0 || sr_out <= 0 || max_samples_in < 1 || batch < 1)
        return twv_fail(TWV_E_INVALID, "bad argument (rates > 0, max_samples_in >= 1, batch >= 1)");
    if (sr_in == sr_out) return twv_fail(TWV_E_INVALID, "equal rates: nothing to resample");
    const long long g = rs_gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g;
    long long W = L >= M ? RS_ZEROS : (RS_ZEROS * M + L - 1) / L;
    W = (W + 3) / 4 * 4;
    const long long taps = 2 * W;
    if (L * taps > RS_TABLE_CAP)
        return twv_fail(TWV_E_UNSUPPORTED, "ratio " + std::to_string(L) + "/" + std::to_string(M) + ": the coefficient table (" + std::to_string(L) +
                        " phases x " + std::to_string(taps) + " taps) exceeds " + std::to_string(RS_TABLE_CAP) + " floats");
    int lr = 0, chunks = 1;
    for (int cand : {64, 16, 4}) {
        if ((long long)cand * M > (1 << 20) || rs_lds_floats((int)L, (int)M, (int)taps, cand) * 4 > RS_LDS_CAP) continue;
        lr = cand;
        break;
    }
    if (!lr) return twv_fail(TWV_E_UNSUPPORTED, "ratio " + std::to_string(L) + "/" + std::to_string(M) + ": a tile of four rounds does not fit the LDS budget");
    while (L * lr * chunks < RS_TILE_OUT && rs_lds_floats((int)L, (int)M, (int)taps, lr * chunks * 2) * 4 <= RS_LDS_GROW) chunks *= 2;
    const long long n_out = ((long long)max_samples_in * L + M - 1) / M;
    const long long tile_out = L * lr * chunks, tiles = (n_out + tile_out - 1) / tile_out;
    if (n_out > 0x7fffffffLL || tiles * batch > 0x7fffffffLL || (long long)max_samples_in * batch > (1LL << 40))
        return twv_fail(TWV_E_INVALID, "batch x samples too large");
    twv_resampler* h = new twv_resampler();
    h->sr_in = sr_in; h->sr_out = sr_out; h->L = (int)L; h->M = (int)M; h->W = (int)W; h->taps = (int)taps;
    h->max_in = max_samples_in; h->batch = batch; h->out_stride = (int)n_out; h->lr = lr; h->chunks = chunks;
    h->lds_bytes = rs_lds_floats(h->L, h->M, h->taps, lr * chunks) * 4;
    h->table_at = nullptr;
    h->name = "rs_resample_kernel<" + std::to_string(lr) + ">";
    const double s = L >= M ? 1.0 : (double)L / (double)M, i0b = rs_i0(RS_BETA);
    h->table.resize((size_t)L * taps);
    for (long long p = 0; p < L; ++p)
        for (long long k = 0; k < taps; ++k) {
            const double u = s * ((double)((k - W) * L + p) / (double)L);
            double c = 0.0;
            if (fabs(u) < RS_ZEROS) {
                const double v = M_PI * RS_ROLLOFF * u, z = u / RS_ZEROS;
                c = s * RS_ROLLOFF * (v == 0.0 ? 1.0 : sin(v) / v) * rs_i0(RS_BETA * sqrt(1.0 - z * z)) / i0b;
            }
            h->table[(size_t)(p * taps + k)] = (float)c;
        }
    *out = h;
    return TWV_OK;
}
extern "C" void twv_resample_destroy(twv_resampler* h) { delete h; }
extern "C" int twv_resample_phases(const twv_resampler* h) { return h->L; }
extern "C" int twv_resample_taps(const twv_resampler* h) { return h->taps; }
extern "C" int64_t twv_resample_out_samples(const twv_resampler* h, int64_t n_in) { return n_in < 0 ? -1 : (int64_t)rs_out_samples(h, n_in); }
extern "C" const char* twv_resample_kernel_name(const twv_resampler* h) { return h->name.c_str(); }
extern "C" int twv_resample_rounds(const twv_resampler* h) { return h->lr * h->chunks; }

static size_t rs_round(size_t n) { return (n + 255) / 256 * 256; }
extern "C" size_t twv_resample_workspace_bytes(const twv_resampler* h)
{
    return rs_round((size_t)h->batch * 8) + rs_round(h->table.size() * 4) + 256;
}
extern "C" int twv_resample_filter_host(const twv_resampler* h, float* out)
{
    if (!h || !out) return twv_fail(TWV_E_INVALID, "bad argument");
    for (size_t i = 0; i < h->table.size(); ++i) out[i] = h->table[i];
    return TWV_OK;
}

extern "C" int twv_resample(twv_resampler* h, const void* in, int in_format, int channels, const int32_t* lengths_host, void* workspace,
                            float* out, void* stream)
{
    if (!h || !in || !workspace || !out) return twv_fail(TWV_E_INVALID, "bad argument");
    if (in_format < 0 || in_format > 1 || channels < 1 || channels > 2)
        return twv_fail(TWV_E_INVALID, "in_format is 0 (float32) or 1 (int16), channels 1 or 2");
    const size_t frame = (size_t)(in_format == 0 ? 4 : 2) * channels;
    if ((uintptr_t)in % frame || (uintptr_t)workspace % 256 || (uintptr_t)out % 4)
        return twv_fail(TWV_E_INVALID, "input not aligned to one frame, or workspace not to 256 bytes");
    h->lengths.resize(2 * (size_t)h->batch);
    for (int b = 0; b < h->batch; ++b) {
        const int len = lengths_host ? lengths_host[b] : h->max_in;
        if (len < 0) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + " has a negative length");
        if (len > h->max_in) return twv_fail(TWV_E_INVALID, "utterance " + std::to_string(b) + " is longer than max_samples_in");
        h->lengths[2 * b] = len;
        h->lengths[2 * b + 1] = (int32_t)rs_out_samples(h, len);
    }
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    int32_t* d_len = (int32_t*)w; w += rs_round((size_t)h->batch * 8);
    float* d_tab = (float*)w;
    if (h->table_at != workspace) {
        HIPCHK(hipMemcpyAsync(d_tab, h->table.data(), h->table.size() * 4, hipMemcpyHostToDevice, st));
        h->table_at = workspace;
    }
    HIPCHK(hipMemcpyAsync(d_len, h->lengths.data(), h->lengths.size() * 4, hipMemcpyHostToDevice, st));
    const long long tile_out = (long long)h->L * h->lr * h->chunks;
    const int tiles = (int)((h->out_stride + tile_out - 1) / tile_out);
    const dim3 grid((unsigned)((long long)tiles * h->batch)), block(RS_THREADS);
#define RS_LAUNCH(LR)                                                                                                                   \
    do {                                                                                                                                \
        if (h->lds_bytes > 32 * 1024)                                                                                                   \
            HIPCHK(hipFuncSetAttribute((const void*)rs_resample_kernel<LR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes)); \
        hipLaunchKernelGGL(rs_resample_kernel<LR>, grid, block, h->lds_bytes, st, in, in_format, channels, d_len, d_tab, out, h->L, h->M, \
                           h->taps, h->chunks, h->max_in, h->out_stride, tiles);                                                        \
    } while (0)
    if (h->lr == 64) RS_LAUNCH(64);
    else if (h->lr == 16) RS_LAUNCH(16);
    else RS_LAUNCH(4);
#undef RS_LAUNCH
    HIPCHK(hipGetLastError());
    return TWV_OK;
}
