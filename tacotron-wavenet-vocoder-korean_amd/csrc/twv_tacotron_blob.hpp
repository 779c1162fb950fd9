// What twv_tacotron_grad.hip needs to know of a twv_tacotron handle (defined in twv_tacotron.hip): its dims and the offsets (floats) of the
// decoder-side tensors in the CANONICAL blob (tacotron.py tacotron_specs order; every tensor row-major as in the checkpoint).  -1 = the
// model has no such tensor (attention_g / attention_b of the un-normalised score, what another attention type owns, layers past
// dec_layer_num).  loc_sen: av = attention_variable, ab = attention_bias; luong_scaled: ag alone.
#pragma once
#include "../../include/twv_amd.h"

// what the recurrent kernels carry by value in their arguments
struct TacoDecoderBlobCore {
    long long Wm, Wq, av, ag, ab, asb;              // memory_layer/kernel, query_layer/kernel, attention_v / _g / _b / _score_bias
    long long dpW1, dpb1, dpW2, dpb2;               // decoder prenet
    long long aWg, abg, aWc, abc;                   // attention GRU: gates / candidate kernel (rows [x | h]) and bias
    long long cW, cb;                               // cell_0 projection
    long long rWg[4], rbg[4], rWc[4], rbc[4];       // residual GRUs
    long long oW, ob;                               // output projection
    long long blob_floats;
};
// with loc_sen's location features, which only its own small kernels read: location_features_convolution/kernel (31, 1, 32), /bias,
// location_features_layer/kernel (32, A)
struct TacoDecoderBlob : TacoDecoderBlobCore {
    long long lcK, lcb, lcL;
};

// The same for one CBHG (twv_tacotron_cbhg_grad.hip): which = 0 the encoder's (with the embedding and the encoder prenet in front of it),
// 1 the post net's (with the linear-spectrogram layer behind it).  A batch_normalization entry is the derived (inv, shift) pair of
// tacotron.flatten: inv at `bn`, shift at `bn` + channels.
struct TacoCbhgBlob {
    int Cin, bank, bch, proj[2], pw, depth, rnn, has_dense;
    long long W[17], b[17], bn[17];                 // conv_bank/conv1d_k, k = 1 .. bank: kernel (k, Cin, bch), bias, batch norm pair
    long long pW[2], pb[2], pbn[2];                 // proj_1, proj_2: kernel (pw, cin, proj[i]), bias, batch norm pair
    long long dW, db;                               // scope/dense (has_dense)
    long long hH[8], hHb[8], hT[8], hTb[8];         // highway layers
    long long gWg[2], gbg[2], gWc[2], gbc[2];       // fw / bw GRU: gates / candidate kernel (rows [x | h]) and bias
    long long emb, pW1, pb1, pW2, pb2;              // encoder only: embedding table, prenet
    long long lW, lb;                               // post net only: the linear-spectrogram layer
    long long blob_floats;
};

const twv_tacotron_dims& taco_dims(const twv_tacotron* h);
void taco_decoder_blob(const twv_tacotron* h, TacoDecoderBlob& b);
void taco_cbhg_blob(const twv_tacotron* h, int which, TacoCbhgBlob& b);
