/*
 * dn_commit.h — C-ABI of the share commitments: SHA-256 of every record of a
 * share wire, and the check of received records against given commitments.
 *
 * Reference interface replaced (delta-mpc/delta-node):
 *   calc_commitment(content)          delta_node/utils/commitment.py:5-12
 * as its callers apply it to one share at a time:
 *   upload_secret_shares              runner/horizontal/agg.py:160-162
 *       commitment = calc_commitment(share), before the share is sealed
 *   get_secret_shares                 runner/horizontal/agg.py:257-272
 *       a received share is kept only if commitment == calc_commitment(share)
 *   the coordinator's checks          coord/horizontal/agg.py:309-318, 342-348
 * A wire is dn_m521_encode_shares' output (dn_shamir.h): records
 * [len(xb)][xb][yb] back to back in `in` with offsets[n + 1]; record e is
 * in[offsets[e], offsets[e + 1]).  Same conventions as dn_shamir.h.
 *
 * Untrusted offsets, by the record-reading entry points' window rule: the 64
 * records e0 .. eN - 1 of a wave (e0 a multiple of 64, eN = min(e0 + 64, n))
 * form the window [offsets[e0], offsets[eN]), usable if offsets[eN] >=
 * offsets[e0] and offsets[eN] <= in_bytes; record e is hashable if its window
 * is usable, offsets[e] >= offsets[e0], offsets[e + 1] >= offsets[e] and
 * offsets[e + 1] <= offsets[eN].  An empty record is hashable (SHA-256 of the
 * empty string, as calc_commitment(b"")).  Whether a record is hashable does
 * not depend on the alignment of `in` or on the size of its window.  Nothing
 * outside in[0, in_bytes), offsets[0, n] and (verify) expect[0, 32 n) is read;
 * nothing outside digests[0, 32 n), ok[0, n) and the two counters is written.
 *
 * Both entry points are one launch without scratch, device table or
 * per-thread state; neither synchronises `stream`, both can be captured into
 * a graph.  n == 0 returns DN_OK and touches no pointer.  DN_ERR_ARG, before
 * any device call: a null required pointer, `in` not 4-byte aligned (a
 * 16-byte aligned wire takes the wide staging path), offsets not 8-byte
 * aligned, digests / expect not 4-byte aligned (16-byte aligned ones are
 * stored / loaded as 16-byte words), digests or ok overlapping in, n of 2^31
 * workgroups (2^39 records) or more.
 */
#ifndef DN_COMMIT_H
#define DN_COMMIT_H

#include <stdint.h>

#include "dn_shamir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* utils/commitment.py:5-12 per record, the sender's side
 * (runner/horizontal/agg.py:160-162): digests[32 e, 32 e + 32) =
 * calc_commitment(record e), bit for bit; 32 zero bytes for a record that is
 * not hashable, counted in bad_counts[0] (ADDED to; [1] is left alone).
 *   in, offsets, digests, bad_counts  DEVICE; bad_counts uint32[2] */
int dn_sha256_commit_records(const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets, uint64_t n,
                             uint8_t* digests, uint32_t* bad_counts /* device uint32[2] */, void* stream);

/* utils/commitment.py:5-12 per record against given commitments, the
 * receiver's and the coordinator's side (runner/horizontal/agg.py:257-272,
 * coord/horizontal/agg.py:309-318, 342-348): record e passes if it is hashable
 * and expect[32 e, 32 e + 32) == calc_commitment(record e).
 *   expect      DEVICE uint8[32 n]
 *   ok          DEVICE uint8[n], 1 where record e passes, else 0; or NULL
 *   bad_counts  DEVICE uint32[2], ADDED to: [0] records that are not hashable
 *               (they do not count in [1]), [1] hashable records whose digest
 *               is not the expected one */
int dn_sha256_verify_records(const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets, uint64_t n,
                             const uint8_t* expect, uint8_t* ok /* or NULL */,
                             uint32_t* bad_counts /* [0] unhashable, [1] mismatches; ADDED to */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DN_COMMIT_H */
