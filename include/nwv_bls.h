/*
 * nwv_bls.h -- BLS12-381 (min_sig) verification on MI355X: SURVEY.md §8 row f4, the reference's
 * default signature scheme.
 *
 * Reference boundary replaced: crypto/src/lib.rs:29-33 aliases PublicKey / Signature /
 * AggregateSignature / PrivateKey / KeyPair to fastcrypto 0.1.2 bls12381::* (Cargo.lock:1534-1561),
 * backed by blst 0.3.10 (Cargo.lock:609-617) in its min_sig flavour: 96-byte compressed G2 public
 * keys, 48-byte compressed G1 signatures, hash to G1 by RFC 9380 under fastcrypto's DST
 * "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_" (NWV_BLS_DST).  The trait contract mirrored is the
 * in-tree template crypto/src/bls12377/mod.rs:264-291 (VerifyingKey) and :485-577
 * (AggregateAuthenticator); the call sites are Header::verify types/src/primary.rs:179-182,
 * Vote::verify :325-327, Certificate::verify :531-534, Certificate::new_unsafe :476-477 and
 * CertificatesResponse::validate_certificates primary/src/block_synchronizer/responses.rs:95-141.
 *
 * Every verification runs on the GPU: signature decode + G1 membership, public-key decode + G2
 * membership (once per device for the keys registered in the key cache below, as fastcrypto
 * validates keys once at deserialization; any other key is decoded by the call that names it),
 * aggregate public key, hash to G1 and the pairing equation e(-sig, g2) e(H(msg), apk) = 1.  By
 * default each item's hash, G1 check and pairing check run on one 64-lane wave each
 * (bls_wave.h: the Miller loop and final exponentiation as lane-parallel stage programs);
 * NWV_FLAG_BLS_BATCH checks all items' equations as one random linear combination instead (one
 * Miller loop per item, one final exponentiation per call; per item only after a rejection).
 * Per-item status codes are exact either way.
 * Buffers are the caller's; the library never retains them.  Thread-safe: concurrent calls on one
 * device run side by side (each takes one of up to eight per-device stream sets).
 */
#ifndef NWV_BLS_H
#define NWV_BLS_H

#include <stddef.h>
#include <stdint.h>

#include "nwv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NWV_BLS_DST "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_"

/* per-item status (the BLST_ERROR subset blst returns on these paths) */
#define NWV_BLS_OK 0
#define NWV_BLS_BAD_ENCODING 1   /* flags / coordinate >= p / stray bits after the infinity flag */
#define NWV_BLS_NOT_ON_CURVE 2   /* x has no y on the curve */
#define NWV_BLS_NOT_IN_GROUP 3   /* signature outside G1 / public key outside G2 */
#define NWV_BLS_AGGR_MISMATCH 4  /* empty key list (or empty aggregation) */
#define NWV_BLS_VERIFY_FAIL 5    /* the pairing equation does not hold */
#define NWV_BLS_PK_INFINITY 6    /* identity public key (or a key sum that is the identity) */

/* The batch entry point (validate_certificates, a DAG round's certificates, the bench): item i is
 * AggregateAuthenticator::verify of the aggregate signature sigs[i] (48 bytes) over the message
 * msg_base[msg_off[i] .. + msg_len[i]) by the keys keys[pk_idx[pk_off[i] + j]], j < pk_cnt[i]
 * (keys: n_keys x 96 bytes, e.g. the committee; a key the device's key cache does not hold is
 * decoded and subgroup-checked once by the call).  status[i] = NWV_BLS_* for item i.  dst = NULL selects NWV_BLS_DST.
 * Returns NWV_OK (statuses valid) or a negative error. */
int nwv_bls_verify_many(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs,
                        const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                        const uint8_t* msg_base, const uint64_t* msg_off, const uint32_t* msg_len,
                        const uint8_t* dst, size_t dst_len, int32_t* status);

/* device time of the last nwv_bls_verify_many call on this context, per stage (HIP events; the
 * first four run on three concurrent streams): [0] keys new to the device's key cache, [1]
 * signature decode + G1 checks, [2] hash to G1, [3] key sums, [4] the pairing check (the batch
 * check k_bls_rlc + k_bls_fold + k_bls_final, plus k_bls_pair when it ran; the whole wave batch
 * check, any per-item re-check included).  Calls of at most
 * 1,024 items record these only on a context opened with NWV_FLAG_BLS_STAGE_TIMES (else zeros). */
int nwv_bls_last_kernel_ms(nwv_ctx* ctx, double out_ms[5]);
/* how the last nwv_bls_verify_many call checked its pairings: 0 per item on the 8-lane group
 * kernels (NWV_FLAG_BLS_PER_ITEM), 1 one batch check that accepted every item and 2 a batch check
 * that rejected, then per item (NWV_FLAG_BLS_BATCH), 3 every item on its own wave (the default) */
int nwv_bls_last_path(nwv_ctx* ctx);
/* two more codes of nwv_bls_last_path, from the wave batch check below: 4 it ran and every group
 * accepted, 5 some group rejected and that group's items were then checked per item */

/* The wave batch check: a large wave call (more than NWV_BLS_WAVE_MAX = 1,024 items, neither
 * NWV_FLAG_BLS_PER_ITEM nor NWV_FLAG_BLS_BATCH) of at least n items -- or a device's share of one,
 * when the context splits the call -- is checked group by group: the items whose decode, G1 and
 * key statuses are OK are split into consecutive groups (env NWV_BLS_BATCH_GROUP items, default
 * 16), every item runs its Miller loop alone, and a group runs ONE final exponentiation over the
 * product of its items' Miller outputs weighted by per-call random 64-bit coefficients.  The items
 * of a group that rejects (and of accepted groups between rejected ones less than 1,024 items
 * apart) run the per-item check, so statuses stay exact.  n = 0 (the
 * default) turns it off: every call then takes exactly the path it takes without this setting.
 * Calls of at most NWV_BLS_WAVE_MAX items never take it whatever n is: they are bound by the
 * latency of one item's chain on one wave, which a shared final exponentiation does not shorten.
 * Every entry point that verifies through nwv_bls_verify_many inherits the setting. */
int nwv_bls_set_wave_batch_min(nwv_ctx* ctx, size_t n);
size_t nwv_bls_wave_batch_min(const nwv_ctx* ctx);
/* the wave batch check of the last nwv_bls_verify_many call: out[0] groups formed, out[1] groups
 * that rejected, out[2] items re-checked per item (zeros when the check did not run) */
int nwv_bls_last_batch(nwv_ctx* ctx, uint64_t out[3]);
/* The key-transposed batch check: the same random linear combination regrouped by registered key.
 * A large wave call (as above) of at least n items -- or a device's share of one -- groups its
 * ELIGIBLE items (decode, G1 and key statuses OK, a signature that is not the identity, every key
 * of the list in the serving device's key cache) into consecutive groups of NWV_BLS_KEY_GROUP
 * items (env, read once; default 2,048).  A group over K distinct keys runs K + 1 Miller loops,
 * each key's on its registered line table, and ONE final exponentiation, whatever its number of
 * items.  A group whose distinct keys + 1 exceed a quarter of its items is not formed (env
 * NWV_BLS_KEY_GROUP_RATIO, read once: the 4 of that rule; 0 forms every group) and its items run
 * the per-item check, as do the OK items that are not eligible and the items of a group that
 * rejects, so statuses stay exact.  When fewer than half of the call's OK items are eligible, or no
 * group is formed, the call takes the path it takes with this setting at 0.  n = 0 (the default)
 * turns it off: every call then takes exactly the launches it takes without this setting.  When
 * this setting and nwv_bls_set_wave_batch_min both qualify, this one runs.  Every entry point that
 * verifies through nwv_bls_verify_many inherits the setting.
 * Two more codes of nwv_bls_last_path: 6 the check ran and every group accepted, 7 some group
 * rejected and its items were then checked per item. */
int nwv_bls_set_key_batch_min(nwv_ctx* ctx, size_t n);
size_t nwv_bls_key_batch_min(const nwv_ctx* ctx);
/* the key-transposed batch check of the calling thread's last nwv_bls_verify_many call (range 0's
 * device when the call split): out[0] groups formed, out[1] groups that rejected, out[2] items of
 * the groups that a per-item launch covered again, out[3] Miller loops the check ran (the groups'
 * key entries plus one signature entry a group), out[4] items in the groups (zeros when the check
 * did not run) */
int nwv_bls_last_key_batch(nwv_ctx* ctx, uint64_t out[5]);
/* The dense key-sum stage.  A large wave call (as above) of at least n items -- or a device's
 * share of one -- sums its items' keys with several items to a wave instead of one wave an item:
 * the items whose keys all sit in the serving device's key cache and whose list names at least two
 * keys get L lanes each (L = 4, 8 or 16: the largest that still fills 65,536 lanes, else 4; env
 * NWV_BLS_APK_LANES, read once, forces one), every other item keeps the per-item kernel.  When
 * every key of the call's key table is registered, an item whose list is strictly ascending and
 * names more than half of the table takes its sum as the table's total minus the keys it leaves
 * out; every other item is summed directly, so repeated and unsorted lists keep their
 * multiplicity.  The sums, and every status, are those of the per-item kernel; the pairing paths
 * (per item, nwv_bls_set_wave_batch_min, nwv_bls_set_key_batch_min) read them unchanged.  n = 0
 * (the default) turns it off: every call then takes exactly the launches it takes without this
 * setting.  Calls of at most NWV_BLS_WAVE_MAX items never take it. */
int nwv_bls_set_apk_dense_min(nwv_ctx* ctx, size_t n);
size_t nwv_bls_apk_dense_min(const nwv_ctx* ctx);
/* the dense key-sum stage of the calling thread's last nwv_bls_verify_many call (range 0's device
 * when the call split): out[0] items summed directly by the dense kernel, out[1] items summed by
 * complement, out[2] items left to the per-item kernel, out[3] lanes an item (zeros when the stage
 * did not run) */
int nwv_bls_last_apk_dense(nwv_ctx* ctx, uint64_t out[4]);
/* keys of the last nwv_bls_verify_many call: out[0] key-list entries found in the key cache,
 * out[1] distinct keys the call decoded itself */
int nwv_bls_last_keys(nwv_ctx* ctx, uint64_t out[2]);

/* The message ring (per device): hashed message points kept by (dst, message), so a message that
 * recurs -- the votes for a header and the certificate built from them sign one 32-byte digest
 * (types/src/primary.rs:351-364, :594-607) -- is hashed to G1 once, and a message known ahead of
 * its signature (a certificate's digest is a function of its header) can be hashed before the
 * call that needs it.  Opt-in: slots = 0 (the default) means no lookups and no publishes, and
 * every call takes exactly the launches it takes without this setting.  The first non-zero value
 * allocates `slots` records (172 bytes each, at most 65,536) on every BLS device object; a later
 * different non-zero value is NWV_ERR_ARG (the buffer never moves); a later 0 switches lookups and
 * publishes off.  Only calls on the small wave path use the ring (at most NWV_BLS_WAVE_MAX and at
 * most 1,024 items, neither NWV_FLAG_BLS_BATCH nor NWV_FLAG_BLS_PER_ITEM), and only messages of at
 * most 64 bytes under a DST of at most 64 bytes are kept.  Statuses never depend on the ring. */
int nwv_bls_set_msg_ring(nwv_ctx* ctx, size_t slots);
size_t nwv_bls_msg_ring(const nwv_ctx* ctx);
/* hash n messages into the ring of EVERY BLS device object (placement may send the later call to
 * any of them); messages the ring holds, duplicates and messages over 64 bytes are skipped.
 * NWV_OK and nothing done when the ring is off.  dst = NULL selects NWV_BLS_DST. */
int nwv_bls_hash_ahead(nwv_ctx* ctx, size_t n, const uint8_t* msg_base, const uint64_t* msg_off,
                       const uint32_t* msg_len, const uint8_t* dst, size_t dst_len);
/* nwv_bls_verify_many that also hashes n_ahead messages ahead_base[ahead_off[j] .. + ahead_len[j])
 * into the ring, beside the call's own work (its critical path does not wait for them).  Ahead
 * message j is kept only if ahead_gate[j] == UINT32_MAX or status[ahead_gate[j]] == NWV_BLS_OK
 * (ahead_gate = NULL: no gates), so a forged header does not fill the ring.  Statuses are exactly
 * those of nwv_bls_verify_many; with the ring off, or on a call that does not use it, the ahead
 * list is ignored. */
int nwv_bls_verify_many_ahead(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n, const uint8_t* sigs,
                              const uint32_t* pk_off, const uint32_t* pk_cnt, const uint32_t* pk_idx,
                              const uint8_t* msg_base, const uint64_t* msg_off, const uint32_t* msg_len,
                              const uint8_t* dst, size_t dst_len, int32_t* status, size_t n_ahead,
                              const uint8_t* ahead_base, const uint64_t* ahead_off, const uint32_t* ahead_len,
                              const uint32_t* ahead_gate);
/* the ring's part in the calling thread's last verify call on this context: out[0] hits whose
 * record was copied (items whose keys are all in the key cache), out[1] hits that ran the h_eff
 * chain on the record, out[2] hashes computed, out[3] slots published for the call's own
 * messages, out[4] ahead messages published.  All zero when the call did not use the ring. */
int nwv_bls_last_msgs(nwv_ctx* ctx, uint64_t out[5]);
/* slot counts of the ring of the device that served the calling thread's last verify call:
 * out[0] held (published under a message), out[1] busy (reserved by a call in flight), out[2]
 * pinned (read by a call in flight) */
int nwv_bls_msg_ring_stats(nwv_ctx* ctx, uint64_t out[3]);

/* The aggregate-key ring (per device): the key side of a recurring signer set.  A certificate's
 * item sums its signers' keys and computes that sum's Miller-loop lines step by step, where a
 * registered key's item reads a table made at registration; a small committee has few quorums and
 * certificates are validated and fetched again, so the ring keeps, per set, the affine sum of the
 * signers' [h_eff] pk records and its line table, and an item whose set is held runs as a one-key
 * item by a registered key.  Opt-in: slots = 0 (the default) means no lookups and no publishes, and
 * every call takes exactly the launches it takes without this setting.  The first non-zero value
 * allocates `slots` records (about 23 KB each, at most 4,096) on every BLS device object; a later
 * different non-zero value is NWV_ERR_ARG (the buffers never move); a later 0 switches lookups and
 * publishes off.  Only calls on the small wave path use the ring (at most NWV_BLS_WAVE_MAX and at
 * most 1,024 items, neither NWV_FLAG_BLS_BATCH nor NWV_FLAG_BLS_PER_ITEM), and only items of 2 to
 * 1,024 keys that are all in the key cache; a set is the sorted list of its keys' cache slots,
 * duplicates kept.  A set is filled at its second sighting (a table of 4 x slots set hashes
 * remembers the first), by the call that sees it, beside that call's pairing check, and kept only
 * if the item verified: a forged aggregate, an identity sum or any other failure publishes
 * nothing.  nwv_bls_keycache_reset empties the ring.  Statuses never depend on the ring. */
int nwv_bls_set_apk_ring(nwv_ctx* ctx, size_t slots);
size_t nwv_bls_apk_ring(const nwv_ctx* ctx);
/* the ring's part in the calling thread's last verify call on this context: out[0] items served
 * from the ring, out[1] items eligible and not found, out[2] of those, sets noted as seen once,
 * out[3] sets this call published.  All zero when the call did not use the ring. */
int nwv_bls_last_apk(nwv_ctx* ctx, uint64_t out[4]);
/* slot counts of the ring of the device that served the calling thread's last verify call:
 * out[0] held (published under a set), out[1] busy (reserved by a call in flight), out[2] pinned
 * (read by a call in flight) */
int nwv_bls_apk_ring_stats(nwv_ctx* ctx, uint64_t out[3]);

/* The committee key cache (per device).  fastcrypto decodes and validates a public key once, at
 * deserialization; nwv_bls_keycache_register does that once per device for the committee's keys
 * (epoch start, Core::change_epoch primary/src/core.rs:592-611) and keeps the records of the keys
 * that are valid.  Verification calls only look keys up: a key the cache does not hold is decoded
 * by the call itself and never takes a slot (an invalid or stray key cannot fill the cache).
 * nwv_bls_keycache_reset (epoch change) drops every slot once the calls in flight finish.  A
 * device keeps at most 65,536 keys; NWV_FLAG_NO_KEYCACHE contexts keep none. */
int nwv_bls_keycache_register(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys);
int nwv_bls_keycache_reset(nwv_ctx* ctx);
/* number of keys the cache holds (>= 0), or a negative error */
int nwv_bls_keycache_size(nwv_ctx* ctx);

/* ---- fastcrypto 0.1.2 trait surface (bls12381 module) ---- */
/* Verifier::verify(&self = pk, msg, sig): NWV_OK or NWV_ERR_SIGNATURE */
int nwv_bls_verify(nwv_ctx* ctx, const uint8_t pk[96], const uint8_t* msg, size_t msg_len, const uint8_t sig[48]);
/* AggregateAuthenticator::verify(&self, pks, msg); sig NULL = an aggregate holding no signature
 * (sig: None) -> NWV_ERR_SIGNATURE */
int nwv_bls_aggregate_verify(nwv_ctx* ctx, const uint8_t* sig48_or_null, const uint8_t* pks, size_t n_pks,
                             const uint8_t* msg, size_t msg_len);
/* VerifyingKey::verify_batch_empty_fail(msg, pks, sigs): NWV_ERR_EMPTY, NWV_ERR_LENGTH, then the
 * signatures are aggregated (each must decode and lie in G1) and verified against the key sum */
int nwv_bls_verify_batch_empty_fail(nwv_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* pks,
                                    size_t n_pks, const uint8_t* sigs, size_t n_sigs);
/* AggregateAuthenticator::batch_verify(sigs, pks_per_sig, msgs): NWV_ERR_LENGTH on any count
 * mismatch, else NWV_OK iff every aggregate verifies over its message and keys */
int nwv_bls_aggregate_batch_verify(nwv_ctx* ctx, size_t n_aggs, const uint8_t* const* sigs48,
                                   const uint8_t* const* pks, const size_t* n_pks, const uint8_t* const* msgs,
                                   const size_t* msg_lens, size_t n_msgs);
/* AggregateAuthenticator::aggregate(sigs): out48 = the sum; NWV_ERR_SIGNATURE if n == 0 or any
 * signature fails to decode / lies outside G1 (*status_or_null = its NWV_BLS_* code) */
int nwv_bls_aggregate(nwv_ctx* ctx, size_t n, const uint8_t* sigs48, uint8_t out48[48], int32_t* status_or_null);

/* ---- key generation, signing and the primitives (synthetic workloads, tests) ---- */
/* pk = sk * g2 compressed (sk: 32 bytes big-endian, < r): the BLS12381KeyPair derivation */
int nwv_bls_keygen_many(nwv_ctx* ctx, size_t n, const uint8_t* sks, uint8_t* pks);
/* sig = sk * H(msg), compressed */
int nwv_bls_sign_many(nwv_ctx* ctx, size_t n, const uint8_t* sks, const uint8_t* msg_base, const uint64_t* msg_off,
                      const uint32_t* msg_len, const uint8_t* dst, size_t dst_len, uint8_t* sigs);
/* H(msg) = hash_to_curve G1 (RFC 9380), uncompressed affine (x || y, 96 bytes big-endian) */
int nwv_bls_hash_to_g1_many(nwv_ctx* ctx, size_t n, const uint8_t* msg_base, const uint64_t* msg_off,
                            const uint32_t* msg_len, const uint8_t* dst, size_t dst_len, uint8_t* out96);
/* e(P_i, Q_i) (P: 96-byte uncompressed G1, Q: 192-byte uncompressed G2 x.c1||x.c0||y.c1||y.c0,
 * all-zero = identity) as 12 big-endian Fp in tower order (576 bytes), = the optimal ate pairing
 * raised to 3 (the final exponentiation's x-chain computes f^(3(p^12-1)/r)) */
int nwv_bls_pairing_many(nwv_ctx* ctx, size_t n, const uint8_t* P96, const uint8_t* Q192, uint8_t* out576);

#ifdef __cplusplus
}
#endif
#endif
