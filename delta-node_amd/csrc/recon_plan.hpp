// recon_plan.hpp — which tensor, and which of its tiles, one global tile of the
// segmented reconstruct is (dn_m521_reconstruct_many).
//
// Every tensor of the list has its own tiled share rows and outputs (256-
// element tiles, the last one partial), so elements of different tensors never
// share a tile and the work space is the global tile range [0, sum_k
// ceil(n_k / 256)): tensor k owns the tiles [tile_begin_k, tile_begin_{k+1}).
// This header holds the arithmetic that turns (table, global tile) into
// (segment, local tile, live lanes, output offsets) — shared by the kernel
// (shamir_m521.hip, reconstruct_many_kernel) and by a host program that checks
// it against a per-element map (tests/host/recon_plan_check.cpp): it is the
// one place where a mistake reads or writes outside a block.  Below it, the
// host's decision whether a reconstruct call takes the five-limb kernels
// (recon_low_eligible; tools/recon_low_check.cpp runs it).  Plain C++: no
// HIP header.
#pragma once

#include <stdint.h>

#include "seg_plan.hpp"

namespace dn {

// One entry per non-empty tensor, in order, then a sentinel with tile_begin =
// the total tile count (its other fields unused).  Device memory; entry 0 has
// tile_begin 0.  The tensor's k share-row bases are entries [k * s, k * s + k)
// of a separate array of device addresses (s = the entry's index).
struct ReconSegEnt {
  uint32_t tile_begin;  // the tensor's first global tile
  uint32_t reserved;
  uint64_t n_elem;
  uint8_t* out_fe;     // tiled vector of vec_bytes(n_elem), or null
  int64_t* out_u64;    // int64[n_elem], or null
  uint32_t* overflow;  // the tensor's counter, or null
};

// The segment that holds global tile t (t < total): the last s in [0, nseg)
// with tile_begin_s <= t.  (Tab: a pointer to ReconSegEnt — the kernel's is in
// the constant address space, so that the table is read by scalar loads.)
template <typename Tab>
DN_SEG_HD uint32_t recon_seg_find(Tab t, uint32_t nseg, uint32_t tile) {
  uint32_t lo = 0, hi = nseg;  // tile_begin[lo] <= tile < tile_begin[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (t[mid].tile_begin <= tile) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The segment of tile `tile` from a cursor on an earlier one (a wave's tiles
// only increase).  (The sentinel's total > tile ends it.)
template <typename Tab>
DN_SEG_HD uint32_t recon_seg_step(Tab t, uint32_t s, uint32_t tile) {
  while (t[s + 1u].tile_begin <= tile) ++s;
  return s;
}

// Local tile lt of a tensor of n elements (lt < ceil(n / 256)):
// every one of its 256 words is an element (the load-ahead path's condition) ...
DN_SEG_HD bool recon_tile_full(uint64_t n_elem, uint32_t lt) {
  return (static_cast<uint64_t>(lt) + 1u) * kSegTile <= n_elem;
}
// ... its word w (< 256) is the tensor's element recon_elem(lt, w), to be read
// and written only where that is below n (recon_live) ...
DN_SEG_HD uint64_t recon_elem(uint32_t lt, uint32_t w) { return static_cast<uint64_t>(lt) * kSegTile + w; }
DN_SEG_HD bool recon_live(uint64_t n_elem, uint32_t lt, uint32_t w) { return recon_elem(lt, w) < n_elem; }
// ... and the tile starts at this byte of a share row or of the tiled output
// (the int64 output's index is recon_elem itself).
DN_SEG_HD uint64_t recon_tile_offset(uint32_t lt) { return static_cast<uint64_t>(lt) * kSegTileBytes; }

// Whether a reconstruct call may take the five-limb path (recon_low.hpp): it
// asks for the int64 words alone (no field output, no overflow counter: that
// one needs every limb, and asking for it is how a caller keeps the full
// validation), the weights are one limb wide with d = 1, and sum |a_i| < 2^24
// (the bound behind recon_low_word's q).  a: the k weights' limbs, `stride`
// u32 apart; *a_sum receives the sum when the call is eligible.  Decided once
// per call on the host; the unrolled kernels cover k = 2..5 (recon_low_covers).
constexpr uint64_t kReconLowMaxSum = 1ull << 24;
DN_SEG_HD bool recon_low_eligible(bool want_u64, bool want_fe, bool want_overflow, int a_limbs, int has_inv, int k,
                                  const uint32_t* a, uint32_t stride, uint32_t* a_sum) {
  if (!want_u64 || want_fe || want_overflow || a_limbs != 1 || has_inv != 0 || k < 1) return false;
  uint64_t sum = 0;
  for (int i = 0; i < k; ++i) sum += a[static_cast<uint64_t>(i) * stride];
  if (sum >= kReconLowMaxSum) return false;
  *a_sum = static_cast<uint32_t>(sum);
  return true;
}
DN_SEG_HD bool recon_low_covers(int k) { return k >= 2 && k <= 5; }

}  // namespace dn
