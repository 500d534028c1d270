// wire_geom_check.cpp — the share wire geometry (csrc/wire_geom.hpp) on the
// host: the relations between its constants as static_asserts, and their
// values printed as "name value" lines for tests/test_wire_geom_host.py to
// compare with what the Python tests assume (wire_edges.py, the frame tests).
#include <cstdio>

#include "frame_plan.hpp"
#include "wire_geom.hpp"

using namespace dn;

static_assert(kMaxRecord == 1 + 8 + 66 && kMaxRecord <= 255, "[len][x <= 8][y <= 66], and a u8 holds the length");
static_assert(kDecWindow == 64 * kMaxRecord + 8, "64 records and the offset of the first inside its dword pair");
static_assert(kWinLimit == kDecWindow + 12, "and the up to 12 more bytes down to the 16-B boundary");
// the staged window [0, kWinLimit) and parse_lds's reads, from dword -1 (the
// clamp at byte -4) to the dword after the last byte, fit a padded row
static_assert(kWinPad >= 8 && kWinPad % 16 == 0, "dwords -1 and 0 before the window; 16-B aligned rows");
static_assert(kDecRowWords % 4 == 0 && 4 * kDecRowWords >= kWinLimit + 4 + 2 * kWinPad, "the decode row holds it");
// every load of the largest LDS-path window has a register
static_assert(64 * 16 * kStageQ >= kWinLimit && 64 * 4 * kStageW >= kWinLimit, "the staging loads cover the window");
static_assert(kStageRegs >= 4 * kStageQ && kStageRegs >= kStageW, "one register per loaded dword");
// the encoder's window: 64 longest records from up to 15 bytes past a 16-B boundary
static_assert(kEncRowWords % 4 == 0 && 4 * kEncRowWords >= 64 * kMaxRecord + 15, "the encode row holds it");
// the scan
static_assert(kScanStage == kScanThreads * kScanRun && kScanThreads % 64 == 0, "one run per thread, whole waves");
static_assert(kScanLdsWords == kScanStage + kScanStage / kScanRun, "one pad word per run");
static_assert(scan_passes(0) == 0 && scan_passes(1) == 1 && scan_passes(kScanStage) == 1 &&
                  scan_passes(kScanStage + 1) == 2,
              "passes");
static_assert(scan_count(kScanStage + 1, 0) == kScanStage && scan_count(kScanStage + 1, 1) == 1, "counts");
// a frame block's total (the largest any scan stages) fits the 32-bit words
static_assert(static_cast<uint64_t>(kFrameElems) * kMaxRecord < (1ull << 32), "staged totals are 32-bit");

int main() {
  std::printf("kMaxRecord %d\n", kMaxRecord);
  std::printf("kWinPad %d\n", kWinPad);
  std::printf("kDecWindow %d\n", kDecWindow);
  std::printf("kWinLimit %d\n", kWinLimit);
  std::printf("kDecRowWords %d\n", kDecRowWords);
  std::printf("kEncRowWords %d\n", kEncRowWords);
  std::printf("kStageQ %d\n", kStageQ);
  std::printf("kStageW %d\n", kStageW);
  std::printf("kStageRegs %d\n", kStageRegs);
  std::printf("kScanThreads %u\n", kScanThreads);
  std::printf("kScanRun %u\n", kScanRun);
  std::printf("kScanStage %u\n", kScanStage);
  std::printf("kScanLdsWords %u\n", kScanLdsWords);
  std::printf("kFrameBlock %u\n", kFrameBlock);
  std::printf("kFrameWord %u\n", kFrameWord);
  return 0;
}
