// twv_wide.hpp -- host-visible interface of the wide generation kernel (twv_wavenet_wide.hip): models whose
// residual_channels R / dilation_channels D are 32, 64 or 128 and not both 32 (wavenet/model.py:8-10 takes any width).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "twv_layout.hpp"

namespace twv {

// Packed layout of a wide model.  Everything is made of the TILE of twv_layout.hpp (64 outputs x 32 terms = one AC-1 chunk).
// conv_filter|conv_gate: output block jb holds filter channels [32 jb, 32 jb + 32) in lanes 0-31 and the gate channels of the SAME
// indices in lanes 32-63, so one wave forms z = tanh(filter) * sigmoid(gate) of its 32 channels without leaving its registers.
// "fg order" below is that order: index jb * 64 + lane.
struct WideLayout {
    int R, D;
    int RC, DC;            // R/32, D/32: chunks per tap of the conv, chunks of dense / skip
    int NFG;               // D/32 filter|gate output blocks
    int NDB;               // ceil(R/64) dense (and causal) output blocks
    long long off_causal;  // scalar input: [NDB][NCA] tiles (K = ifw, R outputs); one-hot: [2][Q][R] as in the checkpoint
    long long off_layer0, layer_stride;
    // within a layer (floats)
    long long l_fg;        // [NFG][2 RC] tiles: chunks 0..RC-1 read x[t-d] (tap 0), RC..2RC-1 read x[t] (tap 1)
    long long l_wd;        // [NDB][DC] tiles
    long long l_sk;        // [NSJ][DC] tiles
    long long l_bfg;       // [NFG][64] conv biases, fg order
    long long l_bd;        // [NDB][64]
    long long l_bs;        // [S]
    // Layout::off_w1 / off_b1 / off_w2 / off_b2 / off_gcemb / off_up / off_meta keep their meaning;
    // Layout::off_lcw / off_gcw: per layer [NFG][NLC | NGC] tiles (lcw_stride / gcw_stride per layer)
};

struct WideLaunch {
    const float* P;
    float* state;                  // per stream: [hist 64][meta 64 ints][ringpos 64 ints][lcprev NL*2D][rings sum(dilation)*R]
    const float* cond;             // [B][NL][2D] gc projections, then [B][T][NL][2D] lc projections, fg order
    const void* first_input;
    const void* forced;
    const void* uniforms;
    void* out;
    int* status;
    float* dbg;                    // optional [B][dbg_steps][NL*(D+R) + Opad]: per layer z (D) | x (R), then the raw outputs
    int dbg_steps;
    int B, T;
    float temperature;
    Layout lay;
    WideLayout wl;
};

inline bool wide_width_ok(int v) { return v == 32 || v == 64 || v == 128; }
// fills wl and the packed offsets of L (L's model fields, NSJ/NCH/NOJ/NCA/NLC/NGC must be set); returns the packed size in floats
long long wide_build_packed_layout(Layout& L, WideLayout& wl, int R, int D);
bool wide_fits_lds(const Layout& L, int R, int D);          // the kernel's LDS map within 160 KiB
int wide_pack(float* packed, const float* blob, const Layout& L, const WideLayout& wl, hipStream_t st);
int wide_condition(const float* P, const Layout& L, const WideLayout& wl, const float* upsampled, const int32_t* gc_ids, int batch,
                   int n_steps, float* cond, hipStream_t st);
int wide_launch(const WideLaunch& a, hipStream_t st);     // TWV_OK or an error code (text via twv_fail)

}  // namespace twv
