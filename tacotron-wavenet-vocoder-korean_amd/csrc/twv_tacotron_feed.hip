// Tacotron feeds (gfx950).  Batch staging: one packed buffer of a batch's ragged arrays -> the padded arrays a training step reads.
//
// The packed buffer is an array of 32-bit words with four sections, each given by its first word:
//   tokens   every utterance's tokens one after the other (int32)
//   mel      every utterance's mel rows one after the other: (sum of frames, num_mels) float32
//   linear   the same for the linear rows: (sum of frames, num_freq) float32
//   table    `batch` rows of twv_tacotron_feed_row (32 bytes): where an utterance's tokens and frames start, how many there are, its
//            speaker id and its loss coefficient.  Offsets are 64-bit and count tokens / frames from the section's start.
// What is written is what datafeeder_tacotron.py:269-309 `_prepare_batch` builds on the host: inputs (N, T_in) and the two targets
// (N, T_out, C) padded with zeros, input_lengths, loss_coeff, speaker_id.  EVERY output element is stored, the padding too.
//
// One thread per output vector of four words (the targets) or per word (the tokens); no atomics, no thread waits for another.  An
// utterance's valid part of a target is contiguous in the output (its first frames * C words) and contiguous in the source, so a vector
// that lies wholly inside it is one 16-byte store fed by one 16-byte load where the source address allows it, or by four dword loads
// where it does not (num_freq = 1025 rows, sections at odd words: the source's alignment differs from utterance to utterance, the
// output's never does -- the outputs must be 16-byte aligned); a vector wholly in the padding is one 16-byte store of zeros; a vector
// across the edge of the valid part or of the utterance goes word by word.  Words are moved as uint32: no float is ever interpreted.
// What hipcc makes of the two source paths for gfx950: ONE global_load_dwordx4 for both -- the target's unaligned access mode lets a
// 16-byte global load start at any dword, so the four dword loads are merged and the alignment test folds away; the lanes of a wave
// then read 1 KiB in one piece, shifted by 4 .. 12 bytes against the 16-byte grid (nine 128-byte lines instead of eight).  The source
// keeps the two paths: that merge is the compiler's to make, and a 16-byte load through a uint4* at another alignment is not C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_dev.hpp"

namespace tf {

using Row = twv_tacotron_feed_row;
static_assert(sizeof(Row) == 32, "twv_tacotron_feed_row is eight 32-bit words");

// word e of a target (N, T_out, C): per = T_out * C
__device__ inline uint32_t tf_word(const uint32_t* __restrict__ sec, const Row* __restrict__ tab, long long per, int C, long long e)
{
    const long long n = e / per, k = e - n * per;
    const Row r = tab[n];
    return k < (long long)r.n_frames * C ? sec[r.frame_offset * C + k] : 0u;
}

// dst (N, T_out, C) <- sec (sum of frames, C): thread i writes words 4 i .. 4 i + 3
__global__ void __launch_bounds__(256) tf_stage_rows_kernel(const uint32_t* __restrict__ sec, const Row* __restrict__ tab, int C, long long per,
                                                            long long total, uint32_t* __restrict__ dst)
{
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= total) return;
    if (e0 + 4 <= total) {
        const long long n = e0 / per, k = e0 - n * per;
        if (k + 4 <= per) {                                    // the vector lies in one utterance
            const Row r = tab[n];
            const long long valid = (long long)r.n_frames * C;
            if (k + 4 <= valid) {
                const uint32_t* s = sec + r.frame_offset * C + k;
                uint4 v;
                if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) v = *reinterpret_cast<const uint4*>(s);
                else { v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3]; }
                *reinterpret_cast<uint4*>(dst + e0) = v;
                return;
            }
            if (k >= valid) {
                *reinterpret_cast<uint4*>(dst + e0) = make_uint4(0u, 0u, 0u, 0u);
                return;
            }
        }
    }
    const long long e1 = e0 + 4 < total ? e0 + 4 : total;
    for (long long e = e0; e < e1; ++e) dst[e] = tf_word(sec, tab, per, C, e);
}

// inputs (N, T_in) <- the tokens; threads 0 .. N - 1 also write their utterance's length, loss coefficient and speaker id
__global__ void __launch_bounds__(256) tf_stage_tokens_kernel(const uint32_t* __restrict__ tokens, const Row* __restrict__ tab, int N, int T_in,
                                                              uint32_t* __restrict__ inputs, int32_t* __restrict__ lengths,
                                                              float* __restrict__ coeff, int32_t* __restrict__ speaker)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * T_in) return;
    const long long n = e / T_in;
    const int k = (int)(e - n * T_in);
    const Row r = tab[n];
    inputs[e] = k < r.n_tokens ? tokens[r.token_offset + k] : 0u;
    if (e < N) {
        const Row q = tab[e];
        lengths[e] = q.n_tokens; coeff[e] = q.loss_coeff; speaker[e] = q.speaker_id;
    }
}

// ---- alignment edits (synthesizer.py:165-190): a pass's alignments (N, T_in, steps) -> the manual_alignments feed (N, steps, T_in) ----
//   mode 0  the transpose
//   mode 1  zeros, then 1 at (argmax_d in[n][e][:], e) for EVERY encoder row e (padded rows too: an all-zero row puts its 1 at step 0)
//   mode 2  the transpose, squared
//   mode 3  the transpose, then that same 1
// A workgroup takes 32 encoder rows of one utterance.  First (modes 1, 3) each of its four waves finds the argmax of eight rows: the lanes
// read a row's `steps` contiguous floats 64 at a time, each keeps the first maximum of its own positions, and a butterfly picks the larger
// value and, of equal values, the smaller step -- numpy's argmax on finite values.  Then 32 x 32 tiles go through LDS: read with the step
// index running along the lanes, written with the encoder row running along them, so both sides move 128-byte pieces.  Every output
// element is stored exactly once; no atomics.
constexpr int kEditRows = 32;
__global__ void __launch_bounds__(256) tf_alignment_edit_kernel(const float* __restrict__ in, int T_in, int steps, int mode, float* __restrict__ out)
{
    __shared__ float tile[kEditRows][kEditRows + 1];
    __shared__ int arg[kEditRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, e0 = blockIdx.x * kEditRows;
    const float* src = in + (long long)n * T_in * steps;
    float* dst = out + (long long)n * steps * T_in;
    if (mode == 1 || mode == 3) {
        for (int r = wave * 8; r < wave * 8 + 8; ++r) {
            const int e = e0 + r;
            float best = -INFINITY; int at = 0x7fffffff;
            if (e < T_in)
                for (int d = lane; d < steps; d += 64) {
                    const float v = src[(long long)e * steps + d];
                    if (v > best) { best = v; at = d; }
                }
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const float ob = __shfl_xor(best, k); const int oa = __shfl_xor(at, k);
                if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
            }
            if (lane == 0) arg[r] = at;
        }
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    for (int d0 = 0; d0 < steps; d0 += kEditRows) {
        if (mode != 1)
            for (int r = ty; r < kEditRows; r += 8)
                if (e0 + r < T_in && d0 + tx < steps) tile[r][tx] = src[(long long)(e0 + r) * steps + d0 + tx];
        __syncthreads();
        for (int c = ty; c < kEditRows; c += 8) {
            const int d = d0 + c, e = e0 + tx;
            if (d < steps && e < T_in) {
                float v = mode == 1 ? 0.0f : tile[tx][c];
                if (mode == 2) v = v * v;
                else if ((mode == 1 || mode == 3) && arg[tx] == d) v = 1.0f;
                dst[(long long)d * T_in + e] = v;
            }
        }
        __syncthreads();
    }
}

}  // namespace tf
using namespace tf;

extern "C" int twv_tacotron_alignment_edit(const float* alignments, int batch, int t_in, int steps, int mode, float* manual_out, void* stream)
{
    if (!alignments || !manual_out) return twv_fail(TWV_E_INVALID, "null argument");
    if (batch < 1 || t_in < 1 || steps < 1) return twv_fail(TWV_E_INVALID, "batch, t_in and steps must be >= 1");
    if (mode < 0 || mode > 3) return twv_fail(TWV_E_INVALID, "mode must be 0 (transpose), 1 (argmax one-hot), 2 (squared) or 3 (argmax set to 1)");
    if (batch > 65535) return twv_fail(TWV_E_INVALID, "batch above 65535");
    hipLaunchKernelGGL(tf_alignment_edit_kernel, dim3((unsigned)((t_in + kEditRows - 1) / kEditRows), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       alignments, t_in, steps, mode, manual_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return twv_fail(TWV_E_HIP, std::string("twv_tacotron_alignment_edit: ") + hipGetErrorString(e));
    return TWV_OK;
}

extern "C" int twv_tacotron_batch_stage(const void* packed, const twv_tacotron_feed_row* table_host, long long packed_words, long long tokens_at,
                                        long long mel_at, long long linear_at, long long table_at, long long total_tokens, long long total_frames,
                                        int batch, int t_in, int t_out, int num_mels, int num_freq, int32_t* inputs, int32_t* input_lengths,
                                        float* mel_targets, float* linear_targets, float* loss_coeff, int32_t* speaker_id, void* stream)
{
    if (!packed || !table_host || !inputs || !input_lengths || !mel_targets || !linear_targets || !loss_coeff || !speaker_id)
        return twv_fail(TWV_E_INVALID, "null argument");
    if (batch < 1 || t_in < 1 || t_out < 1 || num_mels < 1 || num_freq < 1) return twv_fail(TWV_E_INVALID, "batch, t_in, t_out, num_mels and num_freq must be >= 1");
    if (batch > (1 << 20) || t_in > (1 << 20) || t_out > (1 << 20) || num_mels > (1 << 20) || num_freq > (1 << 20))
        return twv_fail(TWV_E_INVALID, "batch, t_in, t_out, num_mels and num_freq above 2^20");
    if ((long long)batch * t_in > (1LL << 38) || (long long)batch * t_out * num_mels > (1LL << 38) || (long long)batch * t_out * num_freq > (1LL << 38))
        return twv_fail(TWV_E_INVALID, "an output above 2^38 words");
    if (total_tokens < 0 || total_frames < 0 || total_tokens > (1LL << 40) || total_frames > (1LL << 40)) return twv_fail(TWV_E_INVALID, "total_tokens / total_frames out of range");
    // the four sections lie inside the buffer
    const long long at[4] = {tokens_at, mel_at, linear_at, table_at};
    const long long words[4] = {total_tokens, total_frames * num_mels, total_frames * num_freq, (long long)batch * 8};
    for (int i = 0; i < 4; ++i)
        if (at[i] < 0 || packed_words < 0 || at[i] > packed_words || words[i] > packed_words - at[i])
            return twv_fail(TWV_E_INVALID, "a section of the packed buffer lies outside its packed_words");
    if ((reinterpret_cast<uintptr_t>(packed) & 15) != 0 || (table_at & 1) != 0)
        return twv_fail(TWV_E_INVALID, "the packed buffer must be 16-byte aligned and its table start at an even word (64-bit offsets)");
    if (((reinterpret_cast<uintptr_t>(mel_targets) | reinterpret_cast<uintptr_t>(linear_targets)) & 15) != 0)
        return twv_fail(TWV_E_INVALID, "mel_targets and linear_targets must be 16-byte aligned");
    // the table, on the host: every utterance's pieces lie inside their sections and fit the padded sizes
    for (int n = 0; n < batch; ++n) {
        const twv_tacotron_feed_row& r = table_host[n];
        if (r.n_tokens < 0 || r.n_frames < 0 || r.token_offset < 0 || r.frame_offset < 0 || r.token_offset > total_tokens ||
            r.n_tokens > total_tokens - r.token_offset || r.frame_offset > total_frames || r.n_frames > total_frames - r.frame_offset)
            return twv_fail(TWV_E_INVALID, "table row " + std::to_string(n) + ": tokens or frames outside their section");
        if (r.n_tokens > t_in) return twv_fail(TWV_E_INVALID, "table row " + std::to_string(n) + ": " + std::to_string(r.n_tokens) + " tokens do not fit t_in = " + std::to_string(t_in));
        if (r.n_frames > t_out) return twv_fail(TWV_E_INVALID, "table row " + std::to_string(n) + ": " + std::to_string(r.n_frames) + " frames do not fit t_out = " + std::to_string(t_out));
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* base = static_cast<const uint32_t*>(packed);
    const Row* tab = reinterpret_cast<const Row*>(base + table_at);
    const long long ntok = (long long)batch * t_in;
    hipLaunchKernelGGL(tf_stage_tokens_kernel, dim3((unsigned)((ntok + 255) / 256)), dim3(256), 0, st, base + tokens_at, tab, batch, t_in,
                       reinterpret_cast<uint32_t*>(inputs), input_lengths, loss_coeff, speaker_id);
    const struct { long long at; int C; float* dst; } targets[2] = {{mel_at, num_mels, mel_targets}, {linear_at, num_freq, linear_targets}};
    for (const auto& t : targets) {
        const long long per = (long long)t_out * t.C, total = per * batch, vecs = (total + 3) / 4;
        hipLaunchKernelGGL(tf_stage_rows_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, base + t.at, tab, t.C, per, total,
                           reinterpret_cast<uint32_t*>(t.dst));
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return twv_fail(TWV_E_HIP, std::string("twv_tacotron_batch_stage: ") + hipGetErrorString(e));
    return TWV_OK;
}
