// What a Tacotron training step needs beside the three gradient passes: the speaker side's gradient (the speaker table and
// its deep_dense layers, or the five get_embed tables of speaker_embedding_size 1), and the two maps between the training vector -- every
// tensor of tacotron_specs with a batch norm as its (4, C) checkpoint tensor -- and the inference blob, which holds the derived
// (inv, shift) pair (tacotron.flatten).  The clip and the Adam update are the WaveNet step's entries on the flat training vector.
//
// The speaker side works on N x speaker_embedding_size inputs: four small launches, every sum in float64 in one fixed order (k, column or
// utterance ascending), no atomics -- equal inputs give equal bits, and a speaker no utterance names gets a row of exact zeros.
#include "twv_tacotron_blob.hpp"
#include "twv_tacotron_grad_common.hpp"

using tgrad::grid_for;

namespace {

constexpr int kSpkLayers = 8;
const float kBnEps = 1e-3f;          // tf.layers.batch_normalization's default epsilon (tacotron.BN_EPS)

// Where the speaker tensors lie in the canonical blob (tacotron.py tacotron_specs: right behind the embedding table, as twv_tacotron.hip's
// taco_build walks them).  kind 0: a single speaker, no such tensors; 1: 'deepvoice' with a speaker embedding -- `table` (num_speakers,
// speaker_embedding_size) and `layers` dense layers of width[i] columns, kernel W[i] and bias b[i]; 2: speaker_embedding_size 1 --
// `layers` tables (num_speakers, width[i]) at W[i]; 3: model_type 'simple' (the table alone).
struct TacoSpeakerBlob {
    int kind, layers, width[kSpkLayers];
    long long table, W[kSpkLayers], b[kSpkLayers];
};
void taco_speaker_blob(const twv_tacotron* h, TacoSpeakerBlob& b)
{
    const twv_tacotron_dims& d = taco_dims(h);
    memset(&b, 0xff, sizeof(b));                    // every offset -1 until set
    b.kind = 0; b.layers = 0;
    for (int i = 0; i < kSpkLayers; ++i) b.width[i] = 0;
    if (d.num_speakers <= 1) return;
    const int SE = d.speaker_embedding_size;
    long long off = (long long)d.n_symbols * d.embedding_size;
    if (d.model_simple && SE != 1) { b.kind = 3; b.table = off; return; }
    b.layers = 3 + d.dec_layer_num;
    for (int i = 0; i < b.layers; ++i) b.width[i] = i == 0 ? d.enc_prenet_sizes[1] : i == 1 ? 2 * d.enc_rnn_size : i == 2 ? d.attention_state_size : d.dec_rnn_size;
    if (SE == 1) {
        b.kind = 2;
        for (int i = 0; i < b.layers; ++i) { b.W[i] = off; off += (long long)d.num_speakers * b.width[i]; }
        return;
    }
    b.kind = 1; b.table = off; off += (long long)d.num_speakers * SE;
    for (int i = 0; i < b.layers; ++i) { b.W[i] = off; off += (long long)SE * b.width[i]; b.b[i] = off; off += b.width[i]; }
}

// the dense layers of a 'deepvoice' model: layer i has width[i] columns, columns col0[i] .. of a row of dz; dy[i] is its cotangent
struct SpkLayers {
    int layers, SE, S, total;
    int width[kSpkLayers], col0[kSpkLayers], ldy[kSpkLayers];
    long long table, W[kSpkLayers], b[kSpkLayers];
    const float* dy[kSpkLayers];
};
// tables to sum rows into: table i is (S, width[i]) at dst[i] of the gradient blob, fed by the rows src[i][n * ld[i] + k]; its elements are
// start[i] .. start[i + 1] of the launch
struct SpkTables {
    int n, S;
    int width[kSpkLayers], ld[kSpkLayers], start[kSpkLayers + 1];
    long long dst[kSpkLayers];
    const float* src[kSpkLayers];
};

__device__ inline int layer_of(const SpkLayers& L, int c)
{
    int i = 0;
    while (i + 1 < L.layers && c >= L.col0[i + 1]) ++i;
    return i;
}
__device__ inline bool speaker_ok(int id, int S) { return id >= 0 && id < S; }

// dz[n][c] = dy / (1 + |z|)^2 with z = e . W_i + b_i recomputed from the blob, e = table[ids[n]] (tacotron.py:76-84, softsign)
__global__ void sg_dz_kernel(const float* blob, const int32_t* ids, int N, SpkLayers L, float* dz)
{
    const long long total = (long long)N * L.total;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(idx / L.total), c = (int)(idx - (long long)n * L.total), i = layer_of(L, c), j = c - L.col0[i], id = ids[n];
        float out = 0.0f;
        if (speaker_ok(id, L.S)) {
            const float* e = blob + L.table + (long long)id * L.SE;
            const float* w = blob + L.W[i] + j;
            double acc = 0.0;
            for (int k = 0; k < L.SE; ++k) acc = fma((double)e[k], (double)w[(long long)k * L.width[i]], acc);
            const double t = 1.0 + fabs(acc + (double)blob[L.b[i] + j]);
            out = (float)((double)L.dy[i][(long long)n * L.ldy[i] + j] / (t * t));
        }
        dz[idx] = out;
    }
}
// dW_i = e^T dz_i (rows k < SE) and db_i = the column sum of dz_i (row k = SE), utterances in order
__global__ void sg_wgrad_kernel(const float* blob, const int32_t* ids, int N, SpkLayers L, const float* dz, float* grad)
{
    const long long total = (long long)(L.SE + 1) * L.total;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(idx / L.total), c = (int)(idx - (long long)k * L.total), i = layer_of(L, c), j = c - L.col0[i];
        double acc = 0.0;
        for (int n = 0; n < N; ++n) {
            const int id = ids[n];
            if (!speaker_ok(id, L.S)) continue;
            const double d = (double)dz[(long long)n * L.total + c];
            acc = k < L.SE ? fma((double)blob[L.table + (long long)id * L.SE + k], d, acc) : acc + d;
        }
        if (k < L.SE) grad[L.W[i] + (long long)k * L.width[i] + j] = (float)acc;
        else grad[L.b[i] + j] = (float)acc;
    }
}
// d_e[n][k] = sum_i sum_j dz_i[n][j] W_i[k][j], layers and columns in order
__global__ void sg_de_kernel(const float* blob, int N, SpkLayers L, const float* dz, float* d_e)
{
    const long long total = (long long)N * L.SE;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(idx / L.SE), k = (int)(idx - (long long)n * L.SE);
        double acc = 0.0;
        for (int i = 0; i < L.layers; ++i) {
            const float* d = dz + (long long)n * L.total + L.col0[i];
            const float* w = blob + L.W[i] + (long long)k * L.width[i];
            for (int j = 0; j < L.width[i]; ++j) acc = fma((double)d[j], (double)w[j], acc);
        }
        d_e[idx] = (float)acc;
    }
}
// table[s][k] = the sum of the rows n with ids[n] = s, utterances in order; no such row: +0
__global__ void sg_table_kernel(const int32_t* ids, int N, SpkTables T, float* grad)
{
    const int total = T.start[T.n];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        int i = 0;
        while (i + 1 < T.n && idx >= T.start[i + 1]) ++i;
        const int r = idx - T.start[i], s = r / T.width[i], k = r - s * T.width[i];
        double acc = 0.0;
        bool any = false;
        for (int n = 0; n < N; ++n)
            if (ids[n] == s) { acc += (double)T.src[i][(long long)n * T.ld[i] + k]; any = true; }
        grad[T.dst[i] + r] = any ? (float)acc : 0.0f;
    }
}

// ---- the training vector <-> the blob.  Batch norm i keeps its pair at off[i] of the blob and its (4, C) tensor at off[i] + 2 * (the
// channels of the batch norms in front of it) of the training vector.
constexpr int kMaxBn = 40;           // two CBHGs of at most 16 bank convolutions and 2 projections
struct BnMap {
    int n, channels[kMaxBn];
    long long off[kMaxBn];
};

// tacotron.bn_inference_vectors, each operation correctly rounded to float32 in its order: a float64 square root or quotient of float32
// operands rounds to the float32 result (53 >= 2 * 24 + 2 bits)
__global__ void tt_refold_kernel(const float* var, BnMap m, long long blob_floats, float* blob)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < blob_floats; p += (long long)gridDim.x * blockDim.x) {
        long long ahead = 0;
        int i = 0;
        while (i < m.n && p >= m.off[i] + 2LL * m.channels[i]) { ahead += 2LL * m.channels[i]; ++i; }
        if (i == m.n || p < m.off[i]) { blob[p] = var[p + ahead]; continue; }
        const int C = m.channels[i], row = (int)((p - m.off[i]) / C), c = (int)(p - m.off[i]) - row * C;
        const float* t = var + m.off[i] + ahead + c;
        const float gamma = t[0], beta = t[C], mean = t[2 * C], variance = t[3 * C];
        const float root = (float)sqrt((double)__fadd_rn(variance, kBnEps));
        const float inv = __fmul_rn((float)(1.0 / (double)root), gamma);
        blob[p] = row == 0 ? inv : __fsub_rn(beta, __fmul_rn(mean, inv));
    }
}
// tacotron.bn_grad_from_inference_pair: d_gamma = rsqrt(var + eps) (d_inv - mean d_shift), d_beta = d_shift, float64 inside; exact zeros for
// the moving statistics; every other range copied
// (batch: the pair's slots already hold (d_gamma, d_beta) of a pass in batch-statistics mode, which are copied)
__global__ void tt_grad_convert_kernel(const float* var, const float* gblob, BnMap m, long long train_floats, int batch, float* gvar)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < train_floats; t += (long long)gridDim.x * blockDim.x) {
        long long ahead = 0;
        int i = 0;
        while (i < m.n && t >= m.off[i] + ahead + 4LL * m.channels[i]) { ahead += 2LL * m.channels[i]; ++i; }
        if (i == m.n || t < m.off[i] + ahead) { gvar[t] = gblob[t - ahead]; continue; }
        const int C = m.channels[i], row = (int)((t - m.off[i] - ahead) / C), c = (int)(t - m.off[i] - ahead) - row * C;
        const float* pair = gblob + m.off[i] + c;
        float out = 0.0f;
        if (batch) out = row < 2 ? pair[row * C] : 0.0f;
        else if (row == 0) {
            const float* raw = var + m.off[i] + ahead + c;
            const double rs = 1.0 / sqrt((double)raw[3 * C] + (double)kBnEps);
            out = (float)(rs * ((double)pair[0] - (double)raw[2 * C] * (double)pair[C]));
        } else if (row == 1) out = pair[C];
        gvar[t] = out;
    }
}

// tf's assign_moving_average without zero-debias on the moving mean and variance of every batch norm: m <- m - (m - batch) * decay, each
// operation rounded to float32.  stats: per batch norm in BnMap order a (2, C) piece = (mean, variance) of the batch
__global__ void tt_moving_update_kernel(float* var, BnMap m, const float* stats, long long total, float decay)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        long long ahead = 0;
        int i = 0;
        while (p >= ahead + 2LL * m.channels[i]) { ahead += 2LL * m.channels[i]; ++i; }
        float* t = var + m.off[i] + ahead + 2LL * m.channels[i] + (p - ahead);       // rows 2, 3 of the (4, C) tensor
        const float v = *t;
        *t = __fsub_rn(v, __fmul_rn(__fsub_rn(v, stats[p]), decay));
    }
}

// dropout multipliers from a counter-based generator: element i of site `site` at step `step` under `seed` depends on those four alone.
//   key = mix(seed + G * (4 * step + site)),  z = mix(key + G * (i + 1)),  u = (z >> 40) * 2^-24   (mix: the splitmix64 finaliser, G its increment)
// kept where u >= rate: out = scale (1 / (1 - rate)) or 0
__device__ __host__ inline unsigned long long tt_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__global__ void tt_dropout_mask_kernel(unsigned long long key, long long total, float rate, float scale, float* out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long z = tt_mix(key + 0x9E3779B97F4A7C15ULL * (unsigned long long)(i + 1));
        const float u = (float)(z >> 40) * 5.9604644775390625e-08f;
        out[i] = u >= rate ? scale : 0.0f;
    }
}

// every batch norm of the model in blob order (the encoder's tensors lie in front of the post net's); returns the floats the training
// vector has more than the blob
long long bn_map(const twv_tacotron* h, BnMap& m)
{
    m.n = 0;
    long long extra = 0;
    for (int which = 0; which < 2; ++which) {
        TacoCbhgBlob c;
        taco_cbhg_blob(h, which, c);
        for (int k = 1; k <= c.bank; ++k) { m.off[m.n] = c.bn[k]; m.channels[m.n++] = c.bch; extra += 2LL * c.bch; }
        for (int i = 0; i < 2; ++i) { m.off[m.n] = c.pbn[i]; m.channels[m.n++] = c.proj[i]; extra += 2LL * c.proj[i]; }
    }
    return extra;
}

// the model's speaker side, or its refusal
int speaker_blob(const twv_tacotron* h, TacoSpeakerBlob& b)
{
    taco_speaker_blob(h, b);
    if (b.kind == 0) return twv_fail(TWV_E_INVALID, "speaker gradient: a single-speaker model has no speaker tensors");
    if (b.kind == 3) return twv_fail(TWV_E_UNSUPPORTED, "model_type 'simple': the speaker gradient is built for 'deepvoice' models");
    return TWV_OK;
}

}  // namespace

extern "C" size_t twv_tacotron_speaker_grad_scratch_bytes(const twv_tacotron* h, int batch)
{
    if (!h || batch < 1) return 0;
    TacoSpeakerBlob b;
    taco_speaker_blob(h, b);
    tgrad::TakeFloats take{nullptr, {}};
    if (b.kind == 1) {
        long long total = 0;
        for (int i = 0; i < b.layers; ++i) total += b.width[i];
        take((long long)batch * total);
        take((long long)batch * taco_dims(h).speaker_embedding_size);
    }
    take(4);
    return (size_t)take.off.used * 4;
}

extern "C" int twv_tacotron_speaker_grad(const twv_tacotron* h, const float* blob, const int32_t* speaker_ids, int batch,
                                         const float* d_before_highway, const float* d_encoder_rnn_init, const float* d_init, void* scratch,
                                         float* grad_blob, void* stream)
{
    if (!h || !blob || !speaker_ids || !d_before_highway || !d_encoder_rnn_init || !d_init || !scratch || !grad_blob)
        return twv_fail(TWV_E_INVALID, "null argument");
    if (batch < 1) return twv_fail(TWV_E_INVALID, "batch >= 1 required");
    TacoSpeakerBlob b;
    GRAD_CHK(speaker_blob(h, b));
    const twv_tacotron_dims& d = taco_dims(h);
    hipStream_t st = (hipStream_t)stream;
    const int N = batch, AS = d.attention_state_size, DR = d.dec_rnn_size, ninit = AS + d.dec_layer_num * DR;
    // the cotangent of layer i, as the forward writes the layer (twv_tacotron.hip, the TACT_SOFTSIGN group)
    const float* dy[kSpkLayers];
    int ldy[kSpkLayers];
    for (int i = 0; i < b.layers; ++i) {
        dy[i] = i == 0 ? d_before_highway : i == 1 ? d_encoder_rnn_init : d_init + (i == 2 ? 0 : AS + (i - 3) * DR);
        ldy[i] = i == 0 ? d.enc_prenet_sizes[1] : i == 1 ? 2 * d.enc_rnn_size : ninit;
    }
    SpkTables T;
    memset(&T, 0, sizeof(T));
    T.S = d.num_speakers;
    if (b.kind == 2) {
        T.n = b.layers;
        for (int i = 0; i < b.layers; ++i) {
            T.width[i] = b.width[i]; T.ld[i] = ldy[i]; T.src[i] = dy[i]; T.dst[i] = b.W[i];
            T.start[i + 1] = T.start[i] + d.num_speakers * b.width[i];
        }
    } else {
        SpkLayers L;
        memset(&L, 0, sizeof(L));
        L.layers = b.layers; L.SE = d.speaker_embedding_size; L.S = d.num_speakers; L.table = b.table;
        for (int i = 0; i < b.layers; ++i) {
            L.width[i] = b.width[i]; L.col0[i] = L.total; L.total += b.width[i]; L.W[i] = b.W[i]; L.b[i] = b.b[i]; L.dy[i] = dy[i]; L.ldy[i] = ldy[i];
        }
        tgrad::TakeFloats take{(float*)scratch, {}};
        float* dz = take((long long)N * L.total);
        float* d_e = take((long long)N * L.SE);
        hipLaunchKernelGGL(sg_dz_kernel, dim3(grid_for((long long)N * L.total)), dim3(256), 0, st, blob, speaker_ids, N, L, dz);
        hipLaunchKernelGGL(sg_wgrad_kernel, dim3(grid_for((long long)(L.SE + 1) * L.total)), dim3(256), 0, st, blob, speaker_ids, N, L, dz, grad_blob);
        hipLaunchKernelGGL(sg_de_kernel, dim3(grid_for((long long)N * L.SE)), dim3(256), 0, st, blob, N, L, dz, d_e);
        T.n = 1; T.width[0] = L.SE; T.ld[0] = L.SE; T.src[0] = d_e; T.dst[0] = b.table; T.start[1] = d.num_speakers * L.SE;
    }
    hipLaunchKernelGGL(sg_table_kernel, dim3(grid_for(T.start[T.n])), dim3(256), 0, st, speaker_ids, N, T, grad_blob);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" size_t twv_tacotron_train_floats(const twv_tacotron* h)
{
    if (!h) return 0;
    BnMap m;
    return (size_t)(twv_tacotron_blob_floats(h) + bn_map(h, m));
}

extern "C" int twv_tacotron_refold(const twv_tacotron* h, const float* variables, float* blob, void* stream)
{
    if (!h || !variables || !blob) return twv_fail(TWV_E_INVALID, "null argument");
    BnMap m;
    bn_map(h, m);
    const long long n = (long long)twv_tacotron_blob_floats(h);
    hipLaunchKernelGGL(tt_refold_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, variables, m, n, blob);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_tacotron_grad_convert(const twv_tacotron* h, const float* variables, const float* grad_blob, float* grad_variables, void* stream)
{
    if (!h || !variables || !grad_blob || !grad_variables) return twv_fail(TWV_E_INVALID, "null argument");
    BnMap m;
    const long long n = (long long)twv_tacotron_blob_floats(h) + bn_map(h, m);
    hipLaunchKernelGGL(tt_grad_convert_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, variables, grad_blob, m, n, 0, grad_variables);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_tacotron_grad_convert_batch(const twv_tacotron* h, const float* grad_blob, float* grad_variables, void* stream)
{
    if (!h || !grad_blob || !grad_variables) return twv_fail(TWV_E_INVALID, "null argument");
    BnMap m;
    const long long n = (long long)twv_tacotron_blob_floats(h) + bn_map(h, m);
    hipLaunchKernelGGL(tt_grad_convert_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)nullptr, grad_blob, m, n, 1, grad_variables);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_tacotron_moving_update(const twv_tacotron* h, float* variables, const float* encoder_stats, const float* post_stats, double momentum,
                                          void* stream)
{
    if (!h || !variables || !encoder_stats || !post_stats) return twv_fail(TWV_E_INVALID, "null argument");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return twv_fail(TWV_E_INVALID, "momentum must lie in [0, 1]");
    BnMap m, part;
    bn_map(h, m);
    const float decay = (float)(1.0 - momentum);
    int first = 0;
    for (int which = 0; which < 2; ++which) {           // one launch per CBHG: its statistics are one buffer, its batch norms a run of the map
        TacoCbhgBlob c;
        taco_cbhg_blob(h, which, c);
        const int n = c.bank + 2;
        long long total = 0, ahead = 0;
        for (int i = 0; i < first; ++i) ahead += 2LL * m.channels[i];
        part.n = n;
        for (int i = 0; i < n; ++i) { part.channels[i] = m.channels[first + i]; part.off[i] = m.off[first + i] + ahead; total += 2LL * part.channels[i]; }
        hipLaunchKernelGGL(tt_moving_update_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, variables, part, which ? post_stats : encoder_stats,
                           total, decay);
        first += n;
    }
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}

extern "C" int twv_dropout_mask(float* out, int64_t n, uint64_t seed, int64_t step, int site, double rate, void* stream)
{
    if (!out) return twv_fail(TWV_E_INVALID, "null argument");
    if (n < 1 || step < 0 || site < 0 || site > 3) return twv_fail(TWV_E_INVALID, "n >= 1, step >= 0 and a site 0 .. 3 required");
    if (!(rate >= 0.0 && rate < 1.0)) return twv_fail(TWV_E_INVALID, "rate must lie in [0, 1)");
    const unsigned long long key = tt_mix((unsigned long long)seed + 0x9E3779B97F4A7C15ULL * (4ULL * (unsigned long long)step + (unsigned long long)site));
    hipLaunchKernelGGL(tt_dropout_mask_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, key, (long long)n, (float)rate, (float)(1.0 / (1.0 - rate)), out);
    GRAD_HIPCHK(hipGetLastError());
    return TWV_OK;
}
