// twv_wavenet_graph.hpp -- host-only: what the WaveNet training step (twv_train.hip) and scoring (twv_score.hip) know in common about
// the train-mode graph (wavenet/model.py:112-167, 247-312): its geometry and the canonical parameter layout, the refusals, the route
// predicates, and the forward front and head that both launch.  Included by those two files only (not by twv_dev.hpp or any header of
// the generation / Tacotron kernels: their hashed source lists do not contain it).
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>
#include <string>
#include "../../include/twv_amd.h"

int twv_fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return twv_fail(TWV_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)
#define BLASCHK(expr)                                                                                             \
    do {                                                                                                          \
        rocblas_status s_ = (expr);                                                                               \
        if (s_ != rocblas_status_success) return twv_fail(TWV_E_HIP, std::string(#expr) + ": rocblas status " + std::to_string((int)s_)); \
    } while (0)

// grid of 256-thread workgroups for a grid-stride loop over n elements
static inline int tg(long long n) { long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 32768 ? 32768 : g)); }

// Geometry of one (rows x samples) batch and the canonical blob offsets: the order of weights.tensor_specs (TF variable order, kernels
// (K, N) row-major).  The ONE place that order is written for the train-mode graph.
struct WavenetLayerOff { long long wf, bf, wg, bg, gcf, gcg, lcf, lcg, wd, bd, ws, bs; };
struct WavenetGraph {
    twv_wavenet_dims d;
    int rows, T, Tn, rf, ow, NL, S, O, L, G, ifw, hop, F;    // rows = batch entries / slots, T samples each, Tn = T - 1, ow = T - rf, F = T / hop frames
    int R, D;                                                // residual / dilation channels: the width (equal; 32, 64 or 128)
    int off[TWV_MAX_LAYERS + 1];                             // receptive offset of layer l's INPUT (off[0] = ifw - 1), off[NL] = rf - 1
    long long c_causal, c_gcemb, c_layer0, c_lstride, c_w1, c_b1, c_w2, c_b2, c_up[4], nparams;
    WavenetLayerOff lo;                                      // offsets inside a layer block
};

// Which kernel families the forward pass runs.  The ONE place these predicates are written: the refusals below, both dispatches and
// both route labels read them here.
enum { WG_LOSS_MOL10 = 0, WG_LOSS_MOLN = 1, WG_LOSS_SOFTMAX = 2 };
struct WavenetRoute {
    bool fused_lc;      // layer kernels on frame-rate lc projections (tr_ctab / tr_mel_shift + one batched GEMM); else the materialised
                        // upsampler (tr_up_fwd) and 80 more k-steps per tile
    bool skinny;        // conv1d_2 as tr_skinny_nn_kernel; else rocBLAS + tr_bias_add_kernel
    int loss;           // WG_LOSS_*
};
inline WavenetRoute wavenet_route(const WavenetGraph& g)
{
    WavenetRoute r;
    r.fused_lc = g.d.n_upsample == 3 && g.hop >= 32 && g.hop <= 512 && g.d.lc_channels == 80;
    const long long RO = (long long)g.rows * g.ow;
    r.skinny = g.O <= 32 && (g.S & 63) == 0 && g.S * 32 * 4 <= 64 * 1024 && RO * g.S * 4 < (1LL << 31);
    r.loss = !g.d.scalar_input ? WG_LOSS_SOFTMAX : (g.O / 3 == 10 ? WG_LOSS_MOL10 : WG_LOSS_MOLN);
    return r;
}
// the part of a route label both handles share; `head` is the caller's word for its head family
inline std::string wavenet_route_label(const WavenetRoute& r, const char* head)
{
    return std::string("lc=") + (r.fused_lc ? "fused" : "staged") + " head=" + head +
           " loss=" + (r.loss == WG_LOSS_MOL10 ? "mol<10>" : r.loss == WG_LOSS_MOLN ? "mol<0>" : "softmax");
}

// Fills g from (dims, rows, samples) and makes every refusal of twv_wavenet_train_create / twv_wavenet_score_create (`what`: "training" /
// "scoring", for the texts).  The width is the caller's to allow: residual_channels = dilation_channels in {32, 64, 128} and at most
// `max_width` (training: twv_wavenet_train_create_w's argument, 32 through twv_wavenet_train_create; scoring: 128).  TWV_OK, or the code twv_fail was given.
inline int wavenet_graph_init(WavenetGraph& g, const twv_wavenet_dims* dims, int rows, int samples, const char* what, int max_width)
{
    const std::string w(what);
    if (dims && dims->gc_channels > 0 && dims->gc_cardinality < 1)
        return twv_fail(TWV_E_UNSUPPORTED, w + " needs global_condition_cardinality (the gc_embedding table is a variable of the graph; model.py:191-195)");
    if (!dims || rows < 1) return twv_fail(TWV_E_INVALID, "bad argument");
    const twv_wavenet_dims& d = *dims;
    if (d.n_layers < 1 || d.n_layers > TWV_MAX_LAYERS || d.n_upsample < 0 || d.n_upsample > 4) return twv_fail(TWV_E_INVALID, "bad dims");
    g.d = d; g.rows = rows; g.T = samples; g.Tn = samples - 1; g.NL = d.n_layers; g.S = d.skip_channels;
    g.O = d.scalar_input ? d.out_channels : d.quantization_channels;
    g.L = d.lc_channels; g.G = d.gc_channels; g.ifw = d.scalar_input ? d.initial_filter_width : 2;   // model.py:36-39
    g.hop = 1;
    for (int i = 0; i < d.n_upsample; ++i) g.hop *= d.upsample_factor[i];
    g.off[0] = g.ifw - 1;
    for (int l = 0; l < g.NL; ++l) g.off[l + 1] = g.off[l] + d.dilations[l];
    g.rf = g.off[g.NL] + 1;
    g.ow = samples - g.rf;                                            // model.py:135 output_width
    g.R = d.residual_channels; g.D = d.dilation_channels;
    if (max_width <= 32) {
        if (g.R != 32 || g.D != 32) return twv_fail(TWV_E_UNSUPPORTED, w + " is built for residual_channels = dilation_channels = 32 only: " + w + " at other widths is not built");
    } else if (g.R != g.D || (g.R != 32 && g.R != 64 && g.R != 128) || g.R > max_width) {
        return twv_fail(TWV_E_UNSUPPORTED, w + " is built for residual_channels = dilation_channels = 32, 64 or 128 only (got " + std::to_string(g.R) + ", " + std::to_string(g.D) + ")");
    }
    if (d.scalar_input && (d.out_channels < 3 || d.out_channels % 3 || d.out_channels > 96)) return twv_fail(TWV_E_UNSUPPORTED, "out_channels must be 3*nr_mix, 3 <= out_channels <= 96");
    if (!d.scalar_input && (d.quantization_channels < 2 || d.quantization_channels > 512)) return twv_fail(TWV_E_UNSUPPORTED, "quantization_channels must be in [2, 512] for " + w);
    if (d.lc_channels != 80 || !d.gc_channels) return twv_fail(TWV_E_UNSUPPORTED, w + " expects num_mels = 80 local and global conditioning (train_vocoder.py, hparams.py:30)");
    // only the FUSED layer kernels (three upsampling stages, 32 <= hop <= 512, 80 mel channels) address a layer's activations with 32-bit
    // byte offsets; the pointer kernels of every other model keep 64-bit addresses and take any size.  Scoring keeps the limit: its
    // memory is bounded by the window batch, a longer utterance is more windows, never a larger batch.  The bound is the same at every
    // width: the wide scoring kernel (sc_layer_wide_fwd_kernel) addresses with 64 bits, so no row it offsets is wider than this one
    if (wavenet_route(g).fused_lc && (long long)rows * samples * 64 * 4 >= (1LL << 31))
        return twv_fail(TWV_E_UNSUPPORTED, w + ": rows x samples too large on the fused lc route: its layer kernels address a layer's activations with 32-bit byte offsets (rows * samples < 8.3 M)");
    if (samples < 1 || samples % g.hop) return twv_fail(TWV_E_INVALID, w + ": the samples per row must be a multiple of the hop size (datafeeder_wavenet.py:38-47)");
    if (g.ow < 1) return twv_fail(TWV_E_INVALID, w + ": the samples per row must exceed the receptive field");
    g.F = samples / g.hop;
    long long c = 0, q = 0;
    const int R = g.R, D = g.D, ub = d.use_biases ? 1 : 0;
    g.c_causal = c; c += d.scalar_input ? (long long)g.ifw * R : 2LL * d.quantization_channels * R;
    g.c_gcemb = c; c += (long long)d.gc_cardinality * g.G;
    g.c_layer0 = c;
    g.lo.wf = q; q += 2 * R * D; g.lo.bf = q; q += ub * D;
    g.lo.wg = q; q += 2 * R * D; g.lo.bg = q; q += ub * D;
    g.lo.gcf = q; q += (long long)g.G * D; g.lo.gcg = q; q += (long long)g.G * D;
    g.lo.lcf = q; q += (long long)g.L * D; g.lo.lcg = q; q += (long long)g.L * D;
    g.lo.wd = q; q += D * R; g.lo.bd = q; q += ub * R;
    g.lo.ws = q; q += (long long)D * g.S; g.lo.bs = q; q += (long long)ub * g.S;
    g.c_lstride = q; c += q * g.NL;
    g.c_w1 = c; c += (long long)g.S * g.S; g.c_b1 = c; c += (long long)ub * g.S;
    g.c_w2 = c; c += (long long)g.S * g.O; g.c_b2 = c; c += (long long)ub * g.O;
    for (int i = 0; i < d.n_upsample; ++i) { g.c_up[i] = c; c += (long long)d.upsample_factor[i] * 2; }
    g.nparams = c;
    return TWV_OK;
}

// The forward front and head, defined in twv_train.hip beside the kernels they launch; each caller fills the pointers from its own carve.
struct WavenetFwdBufs {
    float* ups[5]; const long long* upT;                     // ups[0] = the caller's mel frames, ups[i] = stage i's output (staged route), upT[i] rows each
    float* xunf; int32_t* qin;                               // unfolded audio (scalar input) / mu-law classes (one-hot input)
    float *X0, *emb, *GCP, *WV, *WS, *ctab, *melsh, *Qall;   // layer 0's input, gc embedding rows and projections, weight views, fused-lc tables
    long long vstride, q_ls;                                 // vstride = 2D * (2R + L + G) floats per layer of WV, q_ls = rows * F * 4 * 2D per layer of Qall
    float *ZC, *SK, *C1, *Y;                                 // head: stacked skip input, skip sum, conv1d_1, conv1d_2 outputs
    float* bsum;                                             // S floats of scratch for the summed skip biases
};
// weight views, upsampler stages or ctab / mel shifts / batched Q product, gc gather + batched projection, unfold + causal product or
// mu-law + one-hot causal gather: everything in front of the residual stack
int wavenet_forward_front(const WavenetGraph& g, const float* P, const float* audio, const int32_t* gc_ids, const WavenetFwdBufs& b,
                          rocblas_handle bl, hipStream_t st);
// stacked skip product, bias sum + relu, conv1d_1, conv1d_2 (`skinny`: tr_skinny_nn_kernel, else rocBLAS).  c1_raw: conv1d_1's
// bias + relu pass is not run and C1 keeps pre-activations, which tr_skinny_nn_kernel<true> (and whoever else reads C1) applies to
// what it loads; needs `skinny`
int wavenet_forward_head(const WavenetGraph& g, const float* P, const WavenetFwdBufs& b, bool skinny, bool c1_raw, rocblas_handle bl, hipStream_t st);
