// dn_internal.hpp — shared declarations of the native library (not part of the C-ABI).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "dn_shamir.h"

struct ihipEvent_t;   // hipEvent_t = ihipEvent_t*
struct ihipStream_t;  // hipStream_t = ihipStream_t*

namespace dn {
// A/B tuning knobs (grid cap, wave schedule, store policy, kernel variants).
// The product library is built without DN_TUNING: every knob reads as unset
// and the library consults no environment variable.  `make tuning` builds
// lib/libdn_shamir_tuning.so with -DDN_TUNING, where a knob is the DN_* env
// var of that name, read per call (scripts/ probes and variant tests only).
inline const char* tune_env(const char* name) {
#ifdef DN_TUNING
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// Record a thread-local error message and return `code` (printf-style).
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Forward differences (split by additions) stay below 2^544 while
// sum_{j<t} (n+t)^j < 2^23 (every table entry and every intermediate Newton
// coefficient is bounded by f at some x <= n + t - 1); otherwise the split
// folds after every Horner step.
inline bool fd_needs_fold(int t, int n) {
  double s = 0.0, p = 1.0;
  for (int j = 0; j < t; ++j) {
    s += p;
    p *= static_cast<double>(n + t);
  }
  return s >= 8388608.0;
}

// Compute units of the current device (cached per device; shamir_m521.hip).
int device_cu_count();

// Pinned staging for a table that an entry point uploads WITHOUT synchronising
// its stream (dn_m521_reconstruct_many, dn_m521_encode_shares_many; the pool is
// in shamir_m521.hip).  A buffer carries an event; whoever used it records the
// event on its stream behind the copy before handing the buffer back, and it
// is handed out again only once that event has completed (or to nobody: a busy
// buffer is skipped and a new one made).  So a buffer is never rewritten while
// a copy may still read it, whichever thread or stream asks next: buffers are
// not tied to a stream, and one is in a single call's hands between take() and
// give().  (ev / the stream: hipEvent_t / hipStream_t, named by their
// underlying types so that this header needs no HIP header.)
struct StageBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ::ihipEvent_t* ev = nullptr;
  int dev = -1;
};
// A buffer of at least `need` bytes whose last copy has completed; .p null on failure.
StageBuf stage_take(size_t need);
// Back to the pool; `s`: the stream whose queued copies read the buffer (null
// pointer argument: none were queued).
void stage_give(StageBuf b, ::ihipStream_t* const* s);

// MT19937 jump-ahead (host_mt_jump.cpp): substream length in words, the most
// substreams the jump table covers, a window stepped forward on the host, and
// CPython's final state after `words` outputs (false: beyond the table).
uint64_t mt_jump_words();
uint64_t mt_jump_max_subs();
void mt_advance_window(const uint32_t* win, uint64_t steps, uint32_t* out);
bool mt_final_state(const uint32_t* state, int idx, uint64_t words, uint32_t* fin, int32_t* fidx);

// Runtime direct jump rows (host_gf2poly.cpp): D_s = x^(L - 624 + (s - 1) L)
// mod P, L = 17 * 2^14 words, row s - 1 of kMtPolyWords uint64, for the
// windows a backward-generating draw of S <= kMtRtRows + 1 substreams needs
// (odd s < S and S - 1); computed on first use and cached; *version changes
// whenever rows were added (nullptr: no carry-less multiply on this host, or
// a row disagreed with the tabulated ones).
constexpr uint64_t kMtRtRows = 2048;
const uint64_t* mt_direct_rows_l14(uint64_t S, uint64_t* version);
// D_1 .. D_nrows in sequence into out[nrows][kMtPolyWords] (the build's
// generator of the embedded table, csrc/gen_mt_rt_rows.cpp); false: no
// carry-less multiply, or a row disagreed with the tabulated ones.
bool mt_rt_rows_compute(uint64_t* out, uint64_t nrows);
// out[kMtPolyWords] = x^e mod P (the jump polynomial of e words); false: no
// carry-less multiply on this host
bool mt_xpow_mod(uint64_t e, uint64_t* out);
// The generator's checksum of the embedded table (two words written after it).
void mt_rt_rows_checksum(const uint64_t* words, uint64_t n, uint64_t out[2]);
}  // namespace dn
