// What twv_tacotron_grad.hip needs to know of a twv_tacotron handle (defined in twv_tacotron.hip): its dims and the offsets (floats) of the
// decoder-side tensors in the CANONICAL blob (tacotron.py tacotron_specs order; every tensor row-major as in the checkpoint).  -1 = the
// model has no such tensor (attention_g / attention_b of the un-normalised score, layers past dec_layer_num).
#pragma once
#include "../../include/twv_amd.h"

struct TacoDecoderBlob {
    long long Wm, Wq, av, ag, ab, asb;              // memory_layer/kernel, query_layer/kernel, attention_v / _g / _b / _score_bias
    long long dpW1, dpb1, dpW2, dpb2;               // decoder prenet
    long long aWg, abg, aWc, abc;                   // attention GRU: gates / candidate kernel (rows [x | h]) and bias
    long long cW, cb;                               // cell_0 projection
    long long rWg[4], rbg[4], rWc[4], rbc[4];       // residual GRUs
    long long oW, ob;                               // output projection
    long long blob_floats;
};

const twv_tacotron_dims& taco_dims(const twv_tacotron* h);
void taco_decoder_blob(const twv_tacotron* h, TacoDecoderBlob& b);
