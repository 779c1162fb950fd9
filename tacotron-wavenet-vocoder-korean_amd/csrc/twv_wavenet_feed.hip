// WaveNet crop staging (gfx950): a batch's random crops cut from a corpus that lives on the device.
//
// Two pools of float32 hold the corpus: every example's audio samples (each example starts at a multiple of four floats) and every
// example's mel rows (n_frames, num_mels), packed densely.  A table of 24-byte rows (twv_wavenet_feed_row) says where example i starts in
// each pool, how many frames it has and which speaker it is; `picks` (batch, 2) names, per batch row, the example and the crop's first
// frame.  What is written is what datafeeder_wavenet.py:150-156 cuts on the host: audio (batch, frames * hop) =
// pool[audio_offset + start * hop ...], local_condition (batch, frames, num_mels) = rows start .. start + frames of the example's mels,
// gc_ids (batch) = the speaker ids.
//
// ONE launch; one thread per output vector of four words, the audio's vectors first and the mels' after them; the first `batch` threads
// also write their row's speaker id.  No atomics, no thread waits for another.  A batch row's crop is contiguous in the output and in the
// source, so a vector that lies wholly inside one row is one 16-byte store fed by one 16-byte load where the source address allows it
// (hop 300: every crop starts at a multiple of four floats in the audio pool; the mel pool's rows of 80 floats do too) or by four dword
// loads where it does not (an odd hop, an odd num_mels); a vector across two rows, or across the output's end, goes word by word.  The
// outputs must be 16-byte aligned.  Words are moved as uint32: no float is ever interpreted.  The copy is a few MB and bound by the
// launch; it is not tuned beyond this.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_dev.hpp"

namespace wf {

using Row = twv_wavenet_feed_row;
static_assert(sizeof(Row) == 24, "twv_wavenet_feed_row is six 32-bit words");

// where batch row n's crop starts in its pool, in words: unit = hop (audio) or num_mels (mels)
__device__ inline long long wf_source(const Row* __restrict__ tab, const int32_t* __restrict__ picks, long long n, int unit, bool is_audio)
{
    const Row r = tab[picks[2 * n]];
    return (is_audio ? r.audio_offset : r.mel_offset) + (long long)picks[2 * n + 1] * unit;
}

__global__ void __launch_bounds__(256) wf_crop_kernel(const uint32_t* __restrict__ audio_pool, const uint32_t* __restrict__ mel_pool,
                                                      const Row* __restrict__ tab, const int32_t* __restrict__ picks, int batch,
                                                      long long frames, int hop, int num_mels, long long audio_vecs, long long mel_vecs,
                                                      uint32_t* __restrict__ audio, uint32_t* __restrict__ lc, int32_t* __restrict__ gc)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < batch) gc[i] = tab[picks[2 * i]].speaker_id;
    const bool is_audio = i < audio_vecs;
    if (!is_audio) {
        i -= audio_vecs;
        if (i >= mel_vecs) return;
    }
    const uint32_t* __restrict__ pool = is_audio ? audio_pool : mel_pool;
    uint32_t* __restrict__ dst = is_audio ? audio : lc;
    const int unit = is_audio ? hop : num_mels;
    const long long per = frames * unit, total = per * batch, e0 = i * 4;
    if (e0 + 4 <= total) {
        const long long n = e0 / per, k = e0 - n * per;
        if (k + 4 <= per) {                                    // the vector lies in one batch row
            const uint32_t* s = pool + wf_source(tab, picks, n, unit, is_audio) + k;
            uint4 v;
            if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) v = *reinterpret_cast<const uint4*>(s);
            else { v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3]; }
            *reinterpret_cast<uint4*>(dst + e0) = v;
            return;
        }
    }
    const long long e1 = e0 + 4 < total ? e0 + 4 : total;
    for (long long e = e0; e < e1; ++e) {
        const long long n = e / per;
        dst[e] = pool[wf_source(tab, picks, n, unit, is_audio) + (e - n * per)];
    }
}

}  // namespace wf
using namespace wf;

extern "C" int twv_wavenet_crop_stage(const float* audio_pool, long long audio_floats, const float* mel_pool, long long mel_floats,
                                      const twv_wavenet_feed_row* table_host, const twv_wavenet_feed_row* table_dev, int n_examples,
                                      const int32_t* picks_host, const int32_t* picks_dev, int batch, int frames, int hop_size, int num_mels,
                                      float* audio, float* local_condition, int32_t* gc_ids, void* stream)
{
    if (!audio_pool || !mel_pool || !table_host || !table_dev || !picks_host || !picks_dev || !audio || !local_condition || !gc_ids)
        return twv_fail(TWV_E_INVALID, "null argument");
    if (n_examples < 1 || batch < 1 || frames < 1 || hop_size < 1 || num_mels < 1)
        return twv_fail(TWV_E_INVALID, "n_examples, batch, frames, hop_size and num_mels must be >= 1");
    if (batch > (1 << 20) || frames > (1 << 20) || hop_size > (1 << 20) || num_mels > (1 << 20))
        return twv_fail(TWV_E_INVALID, "batch, frames, hop_size and num_mels above 2^20");
    if ((long long)batch * frames > (1LL << 38) / hop_size || (long long)batch * frames > (1LL << 38) / num_mels)
        return twv_fail(TWV_E_INVALID, "an output above 2^38 words");
    if (audio_floats < 1 || mel_floats < 1 || audio_floats > (1LL << 44) || mel_floats > (1LL << 44))
        return twv_fail(TWV_E_INVALID, "audio_floats / mel_floats out of range");
    if (((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(local_condition)) & 15) != 0)
        return twv_fail(TWV_E_INVALID, "audio and local_condition must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(audio_pool) | reinterpret_cast<uintptr_t>(mel_pool)) & 3)
        return twv_fail(TWV_E_INVALID, "the pools must be 4-byte aligned");
    // the picks and the rows they name, on the host: every crop lies inside its example, every picked example inside its pool
    for (int n = 0; n < batch; ++n) {
        const int ex = picks_host[2 * n], start = picks_host[2 * n + 1];
        const std::string where = "pick " + std::to_string(n) + ": ";
        if (ex < 0 || ex >= n_examples) return twv_fail(TWV_E_INVALID, where + "example " + std::to_string(ex) + " outside [0, " + std::to_string(n_examples) + ")");
        const twv_wavenet_feed_row& r = table_host[ex];
        if (r.n_frames < 0 || r.audio_offset < 0 || r.mel_offset < 0 || r.audio_offset > audio_floats || r.mel_offset > mel_floats ||
            (long long)r.n_frames * hop_size > audio_floats - r.audio_offset || (long long)r.n_frames * num_mels > mel_floats - r.mel_offset)
            return twv_fail(TWV_E_INVALID, where + "the audio or mel range of example " + std::to_string(ex) + " leaves its pool");
        if (start < 0 || start > r.n_frames || frames > r.n_frames - start)
            return twv_fail(TWV_E_INVALID, where + "frames " + std::to_string(start) + " .. " + std::to_string((long long)start + frames) + " outside the " +
                                               std::to_string(r.n_frames) + " frames of example " + std::to_string(ex));
    }
    const long long audio_vecs = ((long long)batch * frames * hop_size + 3) / 4, mel_vecs = ((long long)batch * frames * num_mels + 3) / 4;
    const long long threads = audio_vecs + mel_vecs > batch ? audio_vecs + mel_vecs : batch;
    hipLaunchKernelGGL(wf_crop_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(audio_pool), reinterpret_cast<const uint32_t*>(mel_pool), table_dev, picks_dev, batch,
                       (long long)frames, hop_size, num_mels, audio_vecs, mel_vecs, reinterpret_cast<uint32_t*>(audio),
                       reinterpret_cast<uint32_t*>(local_condition), gc_ids);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return twv_fail(TWV_E_HIP, std::string("twv_wavenet_crop_stage: ") + hipGetErrorString(e));
    return TWV_OK;
}
