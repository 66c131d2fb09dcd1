// The rule by which the read-only reduce (reduce_kernel<REGEN>, kernels_common.hip) REGENERATES part of the noise it
// sums from the key the noise was drawn with, instead of reading it: while the pass streams eps at the HBM floor its
// vector ALUs idle, and every element is sigma * philox_normal4(q, t, u, b, key) -- the function noise_kernel,
// noise_beside_kernel and reduce_kernel<GEN> evaluate bit for bit.  A share of each tile's quads is computed into the
// registers the loads would have filled while the loads of the rest are in flight; the sums, their order and the
// outputs stay what they are.  This header is the only statement of the rule's arithmetic: the engine calls it on the
// host, the kernel on the device, and tests/native/reduce_regen_host.cpp runs it stand-alone.
//
// A tile is kRegenTileQuads quads per lane, quad j of a lane at q0 + 64 j (reduce_kernel's kRU); a row regenerates the
// last n slots of each of its tiles and loads the others.  The share is in eighths of the quads, and n follows from the
// row's place `alt` in a wave's walk over its rows (the waves of a block start one place apart, so at any time a block
// has rows of both kinds in flight): `eighths` of every 8 rows a wave walks are computed entirely, n = 4, the others
// read entirely, n = 0.  A wave is then either streaming with nothing to compute or computing with nothing in flight,
// the waves beside it on the SIMD are in the other state, and the compiler, which sees that n is 0 or 4, emits the two
// kinds of row as two loops without a branch per slot.  Splitting every row's tile instead -- eighths / 2 or
// eighths / 2 + 1 slots computed beside that tile's own loads, alternating from row to row -- was measured and is
// slower at every share.
//
// Regenerating is only ever the same bits where the buffer holds exactly what the plain i.i.d. generator wrote for the
// key recorded beside it, at the pitch being read (content); and it only pays where the pass is bandwidth-bound, the
// reduce's own nontemporal threshold (size).  Content is never overridden; MPPI_REDUCE_REGEN overrides size.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPPI_REGEN_HD __host__ __device__ inline
#else
#define MPPI_REGEN_HD inline
#endif

constexpr int kRegenTileQuads = 4;  // = reduce_kernel's kRU
constexpr int kRegenMaxEighths = 7;
constexpr uint64_t kRegenMinNoiseBytes = 128ull * 1024 * 1024;  // = reduce_kernel's nontemporal threshold
// the share the rule takes where content and size allow (0: the rule is off; DESIGN.md section 4 has the sweep)
constexpr int kRegenDefaultEighths = 2;

// tile slots a row regenerates: all or none; `alt`: the row's place in its wave's walk
MPPI_REGEN_HD int regen_row_quads(int eighths, int alt) { return (alt & 7) < eighths ? kRegenTileQuads : 0; }

// whether tile slot j (0 <= j < kRegenTileQuads) of a row that regenerates n slots is regenerated (else: loaded)
MPPI_REGEN_HD bool regen_slot(int n, int j) { return j >= kRegenTileQuads - n; }

// bytes of one batch's noise [B][nu][H][Kp] fp32
MPPI_REGEN_HD uint64_t regen_noise_bytes(int B, int nu, int H, int Kp) {
  return (uint64_t)B * (uint64_t)nu * (uint64_t)H * (uint64_t)Kp * 4ull;
}

// whether the noise is past the size where the reduce is bandwidth-bound (strictly, as the reduce's own test)
MPPI_REGEN_HD bool regen_size_ok(uint64_t noise_bytes) { return noise_bytes > kRegenMinNoiseBytes; }

// MPPI_REDUCE_REGEN as the rule reads it: -1 unset (or not a digit 0..7), else the digit
MPPI_REGEN_HD int regen_knob(const char* e) {
  if (!e || e[0] < '0' || e[0] > '0' + kRegenMaxEighths || e[1] != '\0') return -1;
  return e[0] - '0';
}

// the rule: the eighths a reduce regenerates.  pristine: the content side (above); knob: regen_knob's value
MPPI_REGEN_HD int regen_share(bool pristine, uint64_t noise_bytes, int knob) {
  if (!pristine || knob == 0) return 0;
  if (knob > 0) return knob <= kRegenMaxEighths ? knob : 0;
  return regen_size_ok(noise_bytes) ? kRegenDefaultEighths : 0;
}
