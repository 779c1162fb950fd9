// twv_wavenet_queue.hip -- the utterance queue's device side: staging of one chunk's inputs from the packed ragged inputs of a list
// of utterances, and collection of the chunk's valid samples into the packed ragged result (DESIGN.md "Utterance queue").
//
// A chunk is `chunk_frames` mel frames (chunk_frames * hop steps) of every slot of a fixed batch.  The schedule is a table uploaded
// once, int32 [n_chunks][batch][4] = {utterance index or -1 (idle), first frame of the piece, valid frames, 1 where the utterance
// starts in this chunk}; `frame_off` (int64 [n_utterances + 1]) holds the prefix sums of the utterances' lengths in frames, which
// place an utterance in every packed array (mel: frames * lc floats; uniforms: frames * hop steps; result: frames * hop samples).
// Two launches per chunk, nothing but copies: 4-byte loads and stores, consecutive lanes on consecutive words, 64-bit offsets (a
// 96-slot batch of 8 s utterances holds more than 2^31 bytes of uniforms).  Steps past an utterance's end and idle slots get the
// padding the generation kernels run on harmlessly: zero mel frames, uniforms 0.5, gc id 0; their samples are never collected.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"
#include "twv_layout.hpp"

using namespace twv;

int twv_fail(int code, const std::string& msg);
const twv::Layout* twv_wavenet_layout_of(const twv_wavenet* h);

namespace {

enum { QT_UTT = 0, QT_FIRST = 1, QT_VALID = 2, QT_START = 3, QT_WORDS = 4 };

struct StageArgs {
    const int32_t* row;           // this chunk's table rows [batch][4]
    const long long* frame_off;   // [n_utterances + 1]
    const uint32_t* mels;         // packed (sum frames, lc) float32
    const uint32_t* uniforms;     // packed (sum frames * hop, wps words): float32 x (nr_mix + 1) | one float64
    const uint32_t* seeds;        // (n_utterances) float32 | int32
    const int32_t* gc_ids;        // (n_utterances) or null
    const uint32_t* prev_out;     // (batch, steps) the previous chunk's output, or null (chunk 0)
    uint32_t* mel_chunk;          // (batch, chunk_frames, lc)
    uint32_t* u_chunk;            // (batch, steps, wps words)
    int32_t* gc_chunk;            // (batch) or null
    uint32_t* first_input;        // (batch)
    int32_t* reset_flags;         // (batch)
    int chunk_frames, hop, lc, wps, pad_float;   // pad_float: uniforms are float32 (0.5f per word), else float64 (0.5 = words {0, 0x3FE00000})
};

// grid (x, batch): slot b's mel words, then its uniform words; thread 0 of block (0, b) writes the slot's scalars
__global__ void __launch_bounds__(256) wn_queue_stage_kernel(StageArgs a)
{
    const int b = blockIdx.y;
    const int32_t* row = a.row + (long long)b * QT_WORDS;
    const int utt = row[QT_UTT], first = row[QT_FIRST], valid = utt >= 0 ? row[QT_VALID] : 0, start = row[QT_START];
    const long long f0 = utt >= 0 ? a.frame_off[utt] + first : 0;              // first frame of the piece in the packed arrays
    const long long steps = (long long)a.chunk_frames * a.hop;
    const long long mel_n = (long long)a.chunk_frames * a.lc, mel_valid = (long long)valid * a.lc;
    const long long u_n = steps * a.wps, u_valid = (long long)valid * a.hop * a.wps;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
    const uint32_t* msrc = a.mels + f0 * a.lc;
    uint32_t* mdst = a.mel_chunk + (long long)b * mel_n;
    for (long long i = tid; i < mel_n; i += nthr) mdst[i] = i < mel_valid ? msrc[i] : 0u;
    const uint32_t* usrc = a.uniforms + f0 * a.hop * a.wps;
    uint32_t* udst = a.u_chunk + (long long)b * u_n;
    for (long long i = tid; i < u_n; i += nthr) {
        const uint32_t pad = a.pad_float ? 0x3F000000u : ((i & 1) ? 0x3FE00000u : 0u);
        udst[i] = i < u_valid ? usrc[i] : pad;
    }
    if (tid == 0) {
        if (a.gc_chunk) a.gc_chunk[b] = (utt >= 0 && a.gc_ids) ? a.gc_ids[utt] : 0;
        // generate.py:204: a continuing utterance is fed the sample just drawn -- the last one of the previous chunk's output, read here
        // on the device; an idle slot is fed zero (silence / class 0)
        uint32_t fi = 0u;
        if (utt >= 0) fi = (start || !a.prev_out) ? a.seeds[utt] : a.prev_out[(long long)b * steps + steps - 1];
        a.first_input[b] = fi;
        a.reset_flags[b] = (utt >= 0 && start) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) wn_queue_collect_kernel(const int32_t* rowp, const long long* frame_off, const uint32_t* out_chunk,
                                                               uint32_t* result, int chunk_frames, int hop)
{
    const int b = blockIdx.y;
    const int32_t* row = rowp + (long long)b * QT_WORDS;
    const int utt = row[QT_UTT];
    if (utt < 0) return;
    const long long steps = (long long)chunk_frames * hop, n = (long long)row[QT_VALID] * hop;
    const uint32_t* src = out_chunk + (long long)b * steps;
    uint32_t* dst = result + (frame_off[utt] + row[QT_FIRST]) * hop;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i];
}

unsigned blocks_for(long long words)
{
    long long g = (words + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

}  // namespace

extern "C" int twv_wavenet_queue_stage(const twv_wavenet* h, const int32_t* table, int chunk, int batch, int chunk_frames,
                                       const int64_t* frame_off, const float* mels, const void* uniforms, const void* seeds,
                                       const int32_t* gc_ids, const void* prev_out, float* mel_chunk, void* u_chunk, int32_t* gc_chunk,
                                       void* first_input, int32_t* reset_flags, void* stream)
{
    const Layout* L = twv_wavenet_layout_of(h);
    if (!L || !table || !frame_off || !mels || !uniforms || !seeds || !mel_chunk || !u_chunk || !first_input || !reset_flags)
        return twv_fail(TWV_E_INVALID, "null argument");
    if (chunk < 0 || batch < 1 || batch > 65535 || chunk_frames < 1) return twv_fail(TWV_E_INVALID, "bad argument");
    if (!L->L) return twv_fail(TWV_E_INVALID, "the utterance queue needs a model with local conditioning (the lengths are those of the mels)");
    StageArgs a;
    a.row = table + (long long)chunk * batch * QT_WORDS;
    a.frame_off = reinterpret_cast<const long long*>(frame_off);
    a.mels = reinterpret_cast<const uint32_t*>(mels); a.uniforms = reinterpret_cast<const uint32_t*>(uniforms);
    a.seeds = reinterpret_cast<const uint32_t*>(seeds); a.gc_ids = gc_ids; a.prev_out = reinterpret_cast<const uint32_t*>(prev_out);
    a.mel_chunk = reinterpret_cast<uint32_t*>(mel_chunk); a.u_chunk = reinterpret_cast<uint32_t*>(u_chunk); a.gc_chunk = gc_chunk;
    a.first_input = reinterpret_cast<uint32_t*>(first_input); a.reset_flags = reset_flags;
    a.chunk_frames = chunk_frames; a.hop = twv_wavenet_hop_size(h); a.lc = L->L;
    a.wps = L->scalar ? L->nr_mix + 1 : 2; a.pad_float = L->scalar ? 1 : 0;
    const long long words = (long long)chunk_frames * ((long long)a.lc + (long long)a.hop * a.wps);
    hipLaunchKernelGGL(wn_queue_stage_kernel, dim3(blocks_for(words), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return twv_fail(TWV_E_HIP, "wn_queue_stage_kernel launch failed");
    return TWV_OK;
}

extern "C" int twv_wavenet_queue_collect(const twv_wavenet* h, const int32_t* table, int chunk, int batch, int chunk_frames,
                                         const int64_t* frame_off, const void* out_chunk, void* result, void* stream)
{
    const Layout* L = twv_wavenet_layout_of(h);
    if (!L || !table || !frame_off || !out_chunk || !result) return twv_fail(TWV_E_INVALID, "null argument");
    if (chunk < 0 || batch < 1 || batch > 65535 || chunk_frames < 1) return twv_fail(TWV_E_INVALID, "bad argument");
    const int hop = twv_wavenet_hop_size(h);
    hipLaunchKernelGGL(wn_queue_collect_kernel, dim3(blocks_for((long long)chunk_frames * hop), (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, table + (long long)chunk * batch * QT_WORDS, reinterpret_cast<const long long*>(frame_off),
                       reinterpret_cast<const uint32_t*>(out_chunk), reinterpret_cast<uint32_t*>(result), chunk_frames, hop);
    if (hipGetLastError() != hipSuccess) return twv_fail(TWV_E_HIP, "wn_queue_collect_kernel launch failed");
    return TWV_OK;
}
