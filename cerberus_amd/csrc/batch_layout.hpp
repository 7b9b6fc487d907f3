// The tables of a batch as the host packs them and the kernels index them: state vector offsets, camera-side dimensions,
// the per-window / per-chunk / per-wave metadata. Plain C++, no HIP: batch_pack.hpp produces these on any host, solver_types.hpp
// hands them to the kernels.
#pragma once
#include "../../include/vilo_gpu.h"

// state vector layout (doubles) per window: vector2double order (estimator.cpp:848-901)
#define XO_POSE 0
#define XO_SB 77
#define XO_LB 176
#define XO_EX 220
#define XO_TD 234
#define XSTRIDE 240

#define CD_EX0 66
#define CD_EX1 72
#define CD_TD 78
#define CD_B0 80
#define CD_N 224  // 80 + 143 = 223, padded

#define CONST_LB 1
#define CONST_EX 2
#define CONST_TD 4

struct WinMeta {
  int n_frames, L, n_chunks, use_leg;
  int lm_off;      // first landmark (device order)
  int chunk_off;   // first group chunk
  int const_mask;
  int prior_n;     // 0: no prior
  int gram_off;    // first Gram slot
  int n_gram;
  int prior_nb;
  int pad;         // frame whose speed/leg-bias block the prior touches (-1: none)
  int wave_off;    // first packed visual wave
  int n_waves;
};

// One wave-sized chunk of the landmarks of a window that share a start frame.
struct ChunkMeta {
  int win, s, n, kmax;      // n <= 64 landmarks, kmax = max observations among them
  int lm_off;               // global device-order index of lane 0
  int lm_local;             // index inside the window
  int gram_off;             // global Gram slot of t = 0 (kmax slots)
  int pad;
  long long obs_off;        // (unused: observations are stored per packed wave, see WaveMeta)
  long long flag_off;
};

// One wave of the visual kernels: up to 4 chunks (different start frames) packed side by side, each starting at a lane
// that is a multiple of 8 (the MFMA Gram pass walks 8 landmarks per trip); observations are stored per wave.
struct WaveMeta {
  int win, nseg, n_lanes, kmax;   // n_lanes: multiple of 8, <= 64; kmax: max over the segments
  int seg_chunk[4];               // global chunk index
  int seg_lane0[4];
  long long obs_off;              // doubles: layout [t][11][n_lanes]
  long long flag_off;             // bytes:   layout [t][n_lanes]  bit0 valid, bit1 stereo
};
