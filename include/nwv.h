/*
 * nwv.h -- C ABI of the MI355X (gfx950) Ed25519 / BLAKE2b-256 verification engine.
 *
 * Drop-in boundary for erwanor/narwhal's signature-verification hot path.  The reference
 * selects its scheme with the five type aliases at crypto/src/lib.rs:29-33 (swap rule
 * :19-27); a GPU-backed Ed25519 scheme module implements the fastcrypto 0.1.2 traits and calls
 * these entry points over FFI (binding stubs: INTEGRATION.md).  Plain pointers and sizes
 * only; the caller owns every buffer; nothing is retained after a call returns.
 *
 * Return codes: NWV_OK (0) on success, NWV_ERR_SIGNATURE (1) when a signature check fails,
 * negative values for usage / runtime errors.  The library never aborts the process.
 * Thread safety: a context may be shared by threads; calls on one device are serialized by
 * a per-device lock.  Every verification call runs on the GPU; if the HIP code object or a
 * device is unavailable nwv_init fails (there is no CPU fallback in this library).
 */
#ifndef NWV_H
#define NWV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWV_OK 0
#define NWV_ERR_SIGNATURE 1      /* verification failed (signature::Error::new())          */
#define NWV_ERR_ARG (-1)         /* bad argument (null pointer, n out of range)             */
#define NWV_ERR_HIP (-2)         /* HIP runtime error                                       */
#define NWV_ERR_OOM (-3)         /* device or host allocation failed                        */
#define NWV_ERR_NODEV (-4)       /* no usable gfx950 device / code object not loadable      */
#define NWV_ERR_EMPTY (-5)       /* verify_batch_empty_fail on an empty batch               */
#define NWV_ERR_LENGTH (-6)      /* |pks| != |sigs| (or messages) in a batch API            */
#define NWV_ERR_REENTRANT (-7)   /* blocking service call made from a completion callback   */

#define NWV_ABI_VERSION 1

typedef struct nwv_ctx nwv_ctx;

/* nwv_init flags.  Batch verification (nwv_ed25519_verify_batch and the trait entry points built
 * on it) runs one Pippenger MSM per device shard (env NWV_MSM_MIN_N sets a minimum shard size,
 * below which the per-signature pipeline runs); these force one or the other. */
#define NWV_FLAG_MSM_ALWAYS 1u
#define NWV_FLAG_MSM_NEVER 2u
/* diagnostic: launch the MSM's hashing (k_msm_scalars) and decompression (k_msm_points) as two
 * kernels instead of one k_msm_prep grid (per-kernel timing of the decompression alone) */
#define NWV_FLAG_MSM_SPLIT_PREP 4u
/* keyed calls (nwv_ed25519_verify_batch_keyed[_digests], the types layer) keep each key's
 * decompressed point and its 2^128 multiple in a per-device cache, so their MSM scalars are
 * 128-bit (half the windows and doublings); this flag turns the cache off (every keyed call
 * decompresses its keys, full-width scalars).  Env NWV_KEYCACHE_MAX_KEYS (default 4096): keyed
 * calls with more distinct keys than this go uncached. */
#define NWV_FLAG_NO_KEYCACHE 8u
/* diagnostic / tests: the batch MSM's two-level counting sort (coarse bins, then each bin in one
 * workgroup) whenever the sort has more than one chunk; by default it is used for windows of
 * NWV_MSM_SORT2_MIN_PTS points or more (env, default 2^20) */
#define NWV_FLAG_MSM_SORT2 16u
/* diagnostic / tests: when a batch MSM over per-signature keys rejects and the verdict bits are
 * wanted, the per-signature pass reuses the MSM's work by default: point tables from its
 * decompressed records (k_ed_points_msm) and k_i / the s < l flag its hash role stored (no
 * k_ed_hash); this flag makes the pass hash and decompress again */
#define NWV_FLAG_NO_MSM_REUSE 32u
/* BLS12-381 (nwv_bls.h): verify every item with its own two-pair Miller loop and final
 * exponentiation on the 8-lane group kernels (round-3 form) instead of the default wave engine --
 * for tests and A/B measurements; statuses are the same either way */
#define NWV_FLAG_BLS_PER_ITEM 64u
/* BLS12-381 (nwv_bls.h): check a call's pairing equations as ONE random linear combination on the
 * 8-lane group kernels (per item only after a rejection) instead of the default, every item's
 * own pairing check on one 64-lane wave (exact per-item statuses either way) */
#define NWV_FLAG_BLS_BATCH 128u
/* BLS12-381 (nwv_bls.h): signatures that passed a verify call of up to 1024 items on the wave path
 * are kept decoded (and G1-checked) on the device, by their 48 bytes, in a ring of 65,536;
 * nwv_bls_aggregate over signatures that are all in it sums the kept points instead of decoding
 * and checking each again (the Core aggregates votes it has already verified).  This flag turns
 * the ring off (every aggregate decodes and checks its signatures). */
#define NWV_FLAG_NO_SIGCACHE 256u
/* diagnostic / tests: small batch MSMs (at most NWV_MSM_ROW_PREP_MAX points to decompress, env,
 * default 8192) run each point's decompression power on a 16-lane row (k_msm_prep's row form,
 * latency-bound batches); this flag keeps every batch on the lane-local decompression */
#define NWV_FLAG_NO_ROW_PREP 512u
/* diagnostic / tests: large host-staged batches (>= 16 MB of pk, sig and messages) start the
 * batch MSM's decompressions -- and, when verdict bits are wanted, the per-signature fallback's
 * tables -- on a second stream once pk and sig are on the device, under the messages' transfer;
 * this flag keeps the one-stream order (every kernel after the whole copy) */
#define NWV_FLAG_NO_EARLY_PREP 1024u
/* diagnostic / tests: a keyed batch MSM whose hashes fit one k_msm_prep workgroup sums its keys'
 * scalars in that workgroup (no k_msm_keysum launch); this flag keeps the separate launch */
#define NWV_FLAG_NO_FUSED_KEYSUM 2048u
/* diagnostic / tests: a keyed batch of at most 64 signatures whose keys were all registered
 * (nwv_keycache_register: each key gets a fixed-base comb table) is checked in one launch,
 * signature by signature (k_ed_tiny), and a larger one of at most nwv_comb_batch_max signatures
 * by the comb kernel (k_ed_comb); this flag sends both through the batch MSM instead */
#define NWV_FLAG_NO_TINY 4096u
/* BLS12-381 calls of at most 1,024 items (the per-call paths) record the per-stage timing events
 * that nwv_bls_last_kernel_ms reports only with this flag: the events cost a single verification
 * ~0.1 ms (larger calls always record them) */
#define NWV_FLAG_BLS_STAGE_TIMES 8192u
/* diagnostic / tests: a per-signature pass of at most nwv_each_row_max signatures (verify_each, or
 * the pass that names the bad set after a rejected batch MSM) runs in one launch of the row kernel
 * (k_ed_each_row); this flag keeps every per-signature pass on the lane pipeline (k_ed_hash,
 * k_ed_points, k_ed_straus) */
#define NWV_FLAG_NO_EACH_ROW 16384u

/* ------------------------------------------------------------------ lifecycle ----- */
/* Process-wide context creation (created once, in Primary::spawn).
 * n_devices: 0 = all visible devices, k = the first k.  flags: NWV_FLAG_* or 0. */
int nwv_init(nwv_ctx** out, int n_devices, uint32_t flags);
/* Context bound to one device ordinal (one process per GPU deployments, bench.py). */
int nwv_init_device(nwv_ctx** out, int device_ordinal, uint32_t flags);
void nwv_free(nwv_ctx* ctx);
int nwv_device_count(const nwv_ctx* ctx);
/* Diagnostics: how the context's batch calls ran so far, summed over its devices: out[0] keyed
 * batches checked by the one-launch path (k_ed_tiny), out[1] batch MSMs, out[2] per-signature
 * passes (verify_each, or after a rejected MSM when verdict bits were asked for). */
int nwv_diag_counters(const nwv_ctx* ctx, uint64_t out[3]);
/* The same with room for later counters: writes the first min(cap, count) counters to out and
 * returns their number, 4 (or an NWV_ERR_* code): the three of nwv_diag_counters, then out[3]
 * registered-key batches checked by the comb kernel (k_ed_comb).  A comb batch counts in neither
 * out[0] nor out[1], and never causes a per-signature pass. */
int nwv_diag_counters_ex(const nwv_ctx* ctx, uint64_t* out, int cap);
/* Largest keyed batch that takes the comb path: a single-device call of more than 64 and at most
 * n signatures whose keys all have a comb table (nwv_keycache_register) is checked signature by
 * signature in one launch of k_ed_comb -- exact ZIP-215 verdict bits, no random coefficients, no
 * fallback pass after a rejection -- unless the context was opened with NWV_FLAG_NO_TINY,
 * NWV_FLAG_MSM_ALWAYS or NWV_FLAG_MSM_NEVER.  0 turns the path off.  A call that splits over
 * several devices keeps the batch MSM, so values at or above the shard minimum (NWV_SHARD_MIN,
 * default 16,384) are clamped to just below it.  The getter returns the value in force. */
int nwv_set_comb_batch_max(nwv_ctx* ctx, size_t n);
size_t nwv_comb_batch_max(const nwv_ctx* ctx);
/* Largest per-signature pass that takes the row kernel: a single-device pass of at most n
 * signatures -- nwv_ed25519_verify_each, or the pass after a rejected batch MSM when verdict bits
 * were asked for, over any keys, registered or not -- runs in one launch of k_ed_each_row (one
 * workgroup a signature, the same exact ZIP-215 verdicts) instead of the three launches of the lane
 * pipeline, unless the context was opened with NWV_FLAG_NO_EACH_ROW or NWV_FLAG_MSM_ALWAYS.
 * Staged batches (nwv_stage_*) always keep the lane pipeline.  Same semantics as
 * nwv_set_comb_batch_max: 0 turns the path off, values at or above the shard minimum are clamped
 * to just below it, the getter returns the value in force. */
int nwv_set_each_row_max(nwv_ctx* ctx, size_t n);
size_t nwv_each_row_max(const nwv_ctx* ctx);
/* Diagnostics, summed over the devices: out[0] per-signature passes run by k_ed_each_row (each of
 * them also counts as a per-signature pass in nwv_diag_counters out[2]), out[1] the signatures in
 * those passes. */
int nwv_diag_each_row(const nwv_ctx* ctx, uint64_t out[2]);
/* How many of those passes ran the reuse form (k_ed_each_row_msm): after a rejected batch MSM over
 * per-signature keys the pass loads the MSM's decompressed R and A records, its k_i and its s < l
 * flags instead of decompressing and hashing again, unless the context was opened with
 * NWV_FLAG_NO_MSM_REUSE.  verify_each and keyed batches always run the plain form. */
int nwv_diag_each_row_reuse(const nwv_ctx* ctx, uint64_t* out);
/* Largest per-signature pass that takes the comb pass kernel: when a single-device keyed batch of
 * more than 64 and at most n signatures whose keys all have a comb table (nwv_keycache_register)
 * goes through the batch MSM and the MSM does not accept it, the pass that names the bad set
 * (verdict bits asked for, or the MSM undetermined) runs in one launch of k_ed_comb_pass -- every
 * signature's [s]B - [k]A summed from B's comb and its key's, the same exact ZIP-215 verdicts --
 * instead of the row kernel or the lane pipeline, unless the context was opened with
 * NWV_FLAG_NO_TINY, NWV_FLAG_MSM_ALWAYS or NWV_FLAG_MSM_NEVER.  An accepted batch launches what it
 * launches without it.  Staged batches (nwv_stage_*) and batches that take k_ed_comb
 * (nwv_set_comb_batch_max) are not affected.  Default 0 (off).  Same semantics as
 * nwv_set_each_row_max: values at or above the shard minimum are clamped to just below it, the
 * getter returns the value in force. */
int nwv_set_comb_pass_max(nwv_ctx* ctx, size_t n);
size_t nwv_comb_pass_max(const nwv_ctx* ctx);
/* Diagnostics, summed over the devices: out[0] per-signature passes run by k_ed_comb_pass (each of
 * them also counts as a per-signature pass in nwv_diag_counters out[2] and
 * nwv_diag_device_counters [8], and never as a comb batch), out[1] the signatures in those passes. */
int nwv_diag_comb_pass(const nwv_ctx* ctx, uint64_t out[2]);
/* Typed calls in one launch.  With a non-zero setting, a call of
 * nwv_ed25519_verify_batch_typed -- and so every Header / Vote / Certificate verification of
 * include/nwv_types.h -- that qualifies runs its digests and its signatures in ONE launch
 * (k_ed_tiny_fused up to 64 signatures, k_ed_comb_fused up to nwv_comb_batch_max) instead of a
 * BLAKE2b launch and a signature launch behind it.  A call qualifies when it is a whole
 * single-device call (fewer signatures than the shard minimum: the setting never applies at or
 * above it), every signing key has a comb table (nwv_keycache_register), no signature is over the
 * digest of a side preimage, and the context was not opened with NWV_FLAG_NO_TINY,
 * NWV_FLAG_MSM_ALWAYS or NWV_FLAG_MSM_NEVER.  Every other call takes the launches it takes with
 * the setting off, and the results are the same bit for bit in both forms.  Default 0 (off). */
int nwv_set_typed_fused(nwv_ctx* ctx, int on);
int nwv_typed_fused(const nwv_ctx* ctx);
/* Diagnostics, summed over the devices: out[0] launches of k_ed_tiny_fused (each also counts as a
 * tiny batch in nwv_diag_counters out[0] and nwv_diag_device_counters [6]), out[1] launches of
 * k_ed_comb_fused (each also a comb batch, nwv_diag_counters_ex [3] and device counter [9]),
 * out[2] typed calls made with the setting on that took the two-launch form. */
int nwv_diag_typed_fused(const nwv_ctx* ctx, uint64_t out[3]);
/* HIP ordinal of the context's i-th device (-1 if out of range) */
int nwv_device_ordinal(const nwv_ctx* ctx, int i);
/* Placement: which device object of a multi-device context serves a call.  A call that does not
 * split (fewer than 2 x NWV_SHARD_MIN signatures; every call the protocol makes) goes to the
 * device with the fewest outstanding ranges, ties to the fewest outstanding items, then to the
 * lowest index, so a caller that issues one call at a time stays on device 0 and only overlapping
 * callers spread.  The ranges of a call that splits rotate over the devices from call to call.  A
 * staged batch counts as one outstanding range on its device from nwv_staged_run until its stream
 * is next synchronised (nwv_staged_sync, nwv_staged_fetch, nwv_staged_free).  Env NWV_PLACE=first
 * (read at nwv_init) keeps a single range on device 0 and range k on device k. */
#define NWV_ENGINE_ED25519 0
#define NWV_ENGINE_BLS 1
/* Placement counters of one device object: writes min(cap, count) values, returns count.
 * [0] ranges placed (a call that does not split is one range)   [1] items in them
 * [2] ranges outstanding now   [3] peak of [2]   [4] HIP ordinal
 * [5] device objects of this engine in the context (replica hooks included)
 * Ed25519 only: [6] tiny  [7] MSM  [8] per-signature  [9] comb batches of this device
 * [0] and [1] count the engine's own calls; [2] and [3] are the device's load, which both engines
 * share when they have the same number of device objects. */
int nwv_diag_device_counters(nwv_ctx* ctx, int engine, int device_index, uint64_t* out, int cap);
/* Latency class (opt-in; 0 = off, the default).  Every call leases a lane -- a stream with its
 * staging and scratch buffers -- of its device object for its whole duration, and waits when all
 * are out.  With a bound n > 0 for an engine, that engine's calls of at most n items are latency
 * class: they take, in order, an idle reserved lane, a new reserved lane (each device object opens
 * up to NWV_LATENCY_LANES of them on demand: env, read at nwv_init, default 2, 1..4), an idle
 * ordinary lane, a new ordinary lane, and otherwise wait for the first lane of either pool.  Every
 * stream of a reserved lane is non-blocking at the greatest priority the device reports (default
 * priority where it reports no range).  All other calls lease from the ordinary lanes only, as
 * without the bound.
 *   NWV_ENGINE_ED25519: signature calls that are one range, n = signatures (verify_each,
 *     verify_batch[_keyed|_grouped], pubkey_verify, the trait surface, the fused
 *     verify_batch_keyed_digests; the types layer and the service through them); digest calls
 *     (nwv_blake2b256_many, nwv_batch_digest_serialized) of at most n messages and at most
 *     NWV_LATENCY_DIGEST_BYTES input bytes in total (env, read at nwv_init, default 1 MiB)
 *   NWV_ENGINE_BLS: nwv_bls_verify_many[_ahead] and nwv_bls_aggregate of at most n items (the
 *     trait surface, the BLS types layer and service through them)
 * Always ordinary: calls that split over devices, nwv_stage_* and staged runs, key-cache
 * registration and retain, signing, key generation, the hash and pairing primitives.
 * Values at or above the engine's shard minimum are clamped to just below it (a latency-class call
 * is always a single range); the getter returns the value in force.  A new value applies to later
 * leases; lanes are never destroyed before nwv_free.  With the bound at 0 no reserved lane and no
 * priority stream is ever created. */
int nwv_set_latency_max(nwv_ctx* ctx, int engine, size_t n);
size_t nwv_latency_max(const nwv_ctx* ctx, int engine);
/* Lane counters of one device object: writes min(cap, count) values, returns count.
 * [0] latency-class calls   [1] of those, the calls that leased a reserved lane
 * [2] of those, the calls that had to wait for any lane
 * [3] all other calls   [4] of those, the calls that waited
 * [5] reserved lanes open   [6] reserved-lane cap   [7] ordinary lanes open */
int nwv_diag_qos(nwv_ctx* ctx, int engine, int device_index, uint64_t* out, int cap);
/* out[0] priority of the reserved lanes' streams, as the runtime reports it for a reserved lane's
 * main stream (0 if none is open yet); out[1] the device's greatest and out[2] its least priority,
 * from the runtime's priority-range query */
int nwv_diag_qos_priority(nwv_ctx* ctx, int engine, int device_index, int out[3]);
int nwv_abi_version(void);
/* last error text for this thread (static storage, never NULL) */
const char* nwv_last_error(void);

/* ------------------------------------------------------------------ Ed25519 --------- */
/* Per-signature ZIP-215 verdicts (ed25519_consensus::VerificationKey::verify semantics for
 * every item; replaces the per-signature verify of types/src/primary.rs:179-182 / :325-327
 * and is the exact-bad-set fallback of primary/src/block_synchronizer/responses.rs:95-141).
 *   pk       n x 32 bytes (compressed A, raw as received: decoding happens here)
 *   sig      n x 64 bytes (R || s)
 *   msg_base message bytes; message i = msg_base[msg_off[i] .. msg_off[i] + msg_len[i])
 *            (a shared message, e.g. a certificate digest, is all msg_off[i] = 0)
 *   verdict_bits  ceil(n/64) words; bit (i % 64) of word i/64 = 1 <=> signature i accepted
 * Work is sharded by contiguous index ranges over the context's devices. */
int nwv_ed25519_verify_each(nwv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig,
                            const uint8_t* msg_base, const uint64_t* msg_off,
                            const uint32_t* msg_len, uint64_t* verdict_bits);

/* Batch verification (ed25519_consensus::batch::Verifier::verify semantics: one verdict for
 * the whole batch).  *all_valid = 1 iff every signature verifies.  seed32 keys the per-batch
 * random coefficients (the caller passes 32 bytes from a CSPRNG; OsRng in the reference).
 * When verdict_bits_or_null is non-NULL and the batch fails, it receives the exact
 * per-signature verdicts (the fallback that pinpoints the bad indices). */
int nwv_ed25519_verify_batch(nwv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig,
                             const uint8_t* msg_base, const uint64_t* msg_off,
                             const uint32_t* msg_len, const uint8_t seed32[32], int* all_valid,
                             uint64_t* verdict_bits_or_null);

/* Batch verification with each verifying key given once: keys (n_keys x 32) and key_idx[n]
 * (signature i is by keys[key_idx[i]]).  ed25519_consensus's batch verifier groups its entries
 * by key the same way (one MSM point per distinct key with coefficient sum z_i k_i), so the
 * device decompresses each distinct key once and carries one point per key instead of one per
 * signature -- the committee case of Certificate::verify / validate_certificates.  Same verdict
 * semantics and outputs as nwv_ed25519_verify_batch. */
int nwv_ed25519_verify_batch_keyed(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, size_t n,
                                   const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg_base,
                                   const uint64_t* msg_off, const uint32_t* msg_len,
                                   const uint8_t seed32[32], int* all_valid, uint64_t* verdict_bits_or_null);
/* Batch verification that finds the repeated keys itself: the arguments, return codes, *all_valid
 * and verdict bits of nwv_ed25519_verify_batch for every input; only the path differs.  This is
 * what the trait-surface calls below run on (they name one key per signature).  The keys are
 * grouped by their 32 bytes on the host -- byte equality, as ed25519_consensus groups by
 * VerificationKeyBytes: two encodings of one point are two keys -- and the call then runs, per
 * range, on the device that serves it:
 *   - every distinct key in that device's key cache: keyed over the cache, so a registered
 *     committee's certificate takes the one-launch path (at most 64 signatures) or the comb kernel
 *     (at most nwv_comb_batch_max), under the conditions of nwv_keycache_register;
 *   - some key not cached, at most n / 2 distinct keys: keyed and uncached (one MSM point per key);
 *   - some key not cached, more distinct keys: exactly as nwv_ed25519_verify_batch.
 * The cache is only looked up: the call never takes a slot and never waits for a fill, so stray
 * keys cannot displace a committee.  The coefficient z_i belongs to the caller's signature i
 * whatever the grouping.  A context opened with NWV_FLAG_MSM_NEVER, and a call of more than
 * NWV_GROUP_MAX_N signatures (env, read once; default 16,384, the shard minimum, so a grouped call
 * is one range and the host pass is bounded), is passed to nwv_ed25519_verify_batch as it is. */
int nwv_ed25519_verify_batch_grouped(nwv_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* sig,
                                     const uint8_t* msg_base, const uint64_t* msg_off,
                                     const uint32_t* msg_len, const uint8_t seed32[32],
                                     int* all_valid, uint64_t* verdict_bits_or_null);
/* Diagnostics: the context's grouped calls so far (n = 0 and argument errors do not count):
 * out[0] calls, out[1] calls that ran with every key from the cache, out[2] calls that ran keyed
 * and uncached, out[3] calls that ran un-keyed (the two pass-through cases included).  A call of
 * several ranges counts once, as its least keyed range; a call that failed counts in out[0] only.
 * Returns NWV_OK or NWV_ERR_ARG. */
int nwv_diag_grouped(const nwv_ctx* ctx, uint64_t out[4]);
/* Digest-then-verify: the n_pre preimages are hashed with BLAKE2b-256 on the
 * device (digests_out receives them, n_pre x 32) and signature i is checked over the 32-byte
 * digest digest_idx[i] straight from device memory, with no host round trip between the hash and
 * the batch verification.  This is how Narwhal signs: a vote's / certificate's signatures are over
 * Vote::digest / Certificate::digest (types/src/primary.rs:351-364, :594-607) and a header's over
 * its id = Header::digest (:209-227).  Otherwise as nwv_ed25519_verify_batch_keyed. */
int nwv_ed25519_verify_batch_keyed_digests(nwv_ctx* ctx, size_t n_pre, const uint8_t* pre_base,
                                           const uint64_t* pre_off, const uint64_t* pre_len,
                                           uint8_t* digests_out, size_t n_keys, const uint8_t* keys,
                                           size_t n, const uint32_t* key_idx, const uint8_t* sig,
                                           const uint32_t* digest_idx, const uint8_t seed32[32],
                                           int* all_valid, uint64_t* verdict_bits_or_null);
/* The typed sibling of nwv_ed25519_verify_batch_keyed_digests: signature i is over message
 * msg_idx[i], where message m < n_pre is the BLAKE2b-256 digest of preimage m and message
 * n_pre + k is the k-th of the n_lit literal 32-byte messages in lits (bytes the caller already
 * holds: a header's id).  pre_short[m] != 0 marks preimage m as a short one: at most 128 bytes (a
 * longer one counts as a side preimage), which the signature kernels may hash themselves; the
 * others are side preimages, hashed for the host (a header's preimage, whose digest only the id
 * comparison reads), and a signature over a side preimage's digest makes the call take the
 * two-launch form.  digests_out receives every digest (n_pre x 32) in both forms; all_valid and
 * the verdict bits are as the sibling's.  With nwv_set_typed_fused the call runs as one launch
 * when it qualifies (see there); otherwise, and on every context with the setting off, it hashes
 * all preimages with the BLAKE2b launch, places the literals behind the digests in the message
 * arena and proceeds as the sibling does, so it is correct at every size. */
int nwv_ed25519_verify_batch_typed(nwv_ctx* ctx, size_t n_pre, const uint8_t* pre_base, const uint64_t* pre_off,
                                   const uint64_t* pre_len, const uint8_t* pre_short, uint8_t* digests_out,
                                   size_t n_lit, const uint8_t* lits, size_t n_keys, const uint8_t* keys,
                                   size_t n, const uint32_t* key_idx, const uint8_t* sig, const uint32_t* msg_idx,
                                   const uint8_t seed32[32], int* all_valid, uint64_t* verdict_bits_or_null);

/* Fill every device's committee key cache with n_keys keys (n_keys x 32), e.g. at epoch start
 * (Core::change_epoch, primary/src/core.rs:592-611).  Batch calls fill the cache themselves;
 * nwv_ed25519_pubkey_verify only looks its key up (an unseen key runs uncached and takes no
 * slot), so registering the committee gives its members' single verifies the cached form.  Each
 * registered key also gets a fixed-base comb table (i 16^j A, 64 KiB), which sends keyed batches
 * of at most 64 signatures by registered keys -- Certificate::verify, Header::verify,
 * Vote::verify -- through the one-launch path, and larger ones of at most nwv_comb_batch_max
 * signatures -- a large committee's certificate, a round's votes, validate_certificates --
 * through the comb kernel.  Registering the same key list again is a no-op.
 * A full cache leaves further keys uncached; verdicts never depend on the cache.  Slots and
 * tables are handed out until nwv_keycache_retain gives some back: call it at every epoch change,
 * before registering the new committee. */
int nwv_keycache_register(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys);
/* Epoch change: on every device of the context, retire every cached key that is NOT in keys
 * (n_keys x 32; n_keys = 0, keys NULL: retire all).  A retired key's slot and comb table are
 * free for later keys.  Registers nothing: call nwv_keycache_register for the new committee
 * afterwards.  out_or_null[4], summed over the devices: [0] slots retired, [1] comb tables
 * retired, [2] slots kept only because a live staged batch reads them, [3] slots in use after
 * (slot 0 included).  Verdicts never depend on it.
 * Keys of the list that are not cached are ignored, duplicates are allowed, and slot 0 (the
 * basepoint) is never retired.  Validators that stay keep their records and tables.  The call
 * waits for the keyed calls in flight on each device (they hold the cache until their kernels
 * have finished) and new ones wait for it, so it completes under continuous callers.  A staged
 * keyed batch (nwv_stage_ed25519_keyed) pins the slots it reads until nwv_staged_free: its keys
 * are kept, with their tables, and go at the first retain after it is freed.  If a retired key
 * belonged to the last fully registered list, registering that list again does the work again.
 * A context opened with NWV_FLAG_NO_KEYCACHE: a successful no-op, out all zero. */
int nwv_keycache_retain(nwv_ctx* ctx, size_t n_keys, const uint8_t* keys, uint64_t* out_or_null);
/* Diagnostics: the key cache of the context's device_index-th device, read under the cache's
 * lock: out[0] slots in use now (slot 0, the basepoint's, included; 0 before the first fill;
 * retired slots do not count), out[1] slot capacity (0 before the cache is allocated), out[2]
 * comb tables in use now, out[3] comb-table
 * capacity (env NWV_COMB_KEYS, default 1,024; 0 before the first registration).  Returns the
 * number of values, 4, or an NWV_ERR_* code (null context, index out of range). */
int nwv_keycache_stats(const nwv_ctx* ctx, int device_index, uint64_t out[4]);

/* ---- fastcrypto 0.1.2 trait surface (Ed25519 scheme module; contract of
 *      crypto/src/bls12377/mod.rs:264-291 and :485-577) ---- */
/* The three batch calls below run on nwv_ed25519_verify_batch_grouped: with the committee
 * registered (nwv_keycache_register, once at start-up and at every epoch change) they reach the
 * cached, one-launch and comb paths with no other change at the call sites. */
/* Verifier::verify(&self, msg, sig): NWV_OK or NWV_ERR_SIGNATURE */
int nwv_ed25519_pubkey_verify(nwv_ctx* ctx, const uint8_t pk[32], const uint8_t* msg,
                              size_t msg_len, const uint8_t sig[64]);
/* VerifyingKey::verify_batch_empty_fail(msg, pks, sigs): NWV_ERR_EMPTY if n_sigs == 0,
 * NWV_ERR_LENGTH if n_pks != n_sigs, else NWV_OK / NWV_ERR_SIGNATURE */
int nwv_ed25519_verify_batch_empty_fail(nwv_ctx* ctx, const uint8_t* msg, size_t msg_len,
                                        const uint8_t* pks, size_t n_pks, const uint8_t* sigs,
                                        size_t n_sigs, const uint8_t seed32[32]);
/* AggregateAuthenticator::verify(&self, pks, msg) for Ed25519AggregateSignature (the
 * aggregate is the list of signatures): NWV_ERR_LENGTH if n_pks != n_sigs */
int nwv_ed25519_aggregate_verify(nwv_ctx* ctx, const uint8_t* sigs, size_t n_sigs,
                                 const uint8_t* pks, size_t n_pks, const uint8_t* msg,
                                 size_t msg_len, const uint8_t seed32[32]);
/* AggregateAuthenticator::batch_verify(sigs, pks_iters, msgs): n_aggs aggregates; aggregate
 * a has n_sigs[a] signatures at sigs[a], n_pks[a] keys at pks[a] and message msgs[a].  Every
 * length mismatch -> NWV_ERR_LENGTH before any crypto. */
int nwv_ed25519_aggregate_batch_verify(nwv_ctx* ctx, size_t n_aggs, const uint8_t* const* sigs,
                                       const size_t* n_sigs, const uint8_t* const* pks,
                                       const size_t* n_pks, const uint8_t* const* msgs,
                                       const size_t* msg_lens, size_t n_msgs,
                                       const uint8_t seed32[32]);

/* ------------------------------------------------------------------ BLAKE2b-256 ------ */
/* fastcrypto::blake2b_256 (VarBlake2b::new(32)) of n independent inputs
 * (types/src/primary.rs:65-73 Batch::digest over pre-concatenated tx bytes, :209-227,
 * :351-364, :594-607 header / vote / certificate digests).  out: n x 32 bytes. */
int nwv_blake2b256_many(nwv_ctx* ctx, size_t n, const uint8_t* base, const uint64_t* off,
                        const uint64_t* len, uint8_t* out);
/* serialized_batch_digest (types/src/worker.rs:44-80) of n bincode WorkerMessage::Batch
 * buffers.  out: n x 32; err_offset[i] = -1 on success, else the byte offset reported by
 * DigestError::InvalidArgumentError.  Returns NWV_OK if all succeeded, NWV_ERR_ARG otherwise. */
int nwv_batch_digest_serialized(nwv_ctx* ctx, size_t n, const uint8_t* base, const uint64_t* off,
                                const uint64_t* len, uint8_t* out, int64_t* err_offset);

/* ------------------------------------------------------------------ resident batches --- */
/* Device-resident staging for throughput measurement and pipelined callers: the inputs are
 * copied to HBM once (SoA: pk, sig, message arena), then verified repeatedly without host
 * traffic.  One staged batch lives on one device of the context. */
typedef struct nwv_staged nwv_staged;
int nwv_stage_ed25519(nwv_ctx* ctx, int device_index, size_t n, const uint8_t* pk,
                      const uint8_t* sig, const uint8_t* msg_base, const uint64_t* msg_off,
                      const uint32_t* msg_len, nwv_staged** out);
/* keyed form (see nwv_ed25519_verify_batch_keyed): mode-1 runs carry one MSM point per key */
int nwv_stage_ed25519_keyed(nwv_ctx* ctx, int device_index, size_t n_keys, const uint8_t* keys, size_t n,
                            const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg_base,
                            const uint64_t* msg_off, const uint32_t* msg_len, nwv_staged** out);
/* mode 0: per-signature verdicts (K1-K4); mode 1: batch verdict through one Pippenger MSM (K5),
 * coefficients keyed by seed32 (NULL: OS entropy).  Asynchronous on the batch's own stream;
 * nwv_staged_sync waits.  Verdicts stay on the device until nwv_staged_fetch, which after a
 * rejected mode-1 run also runs the per-signature fallback (exact bad indices). */
int nwv_staged_run(nwv_staged* st, int mode, const uint8_t seed32[32]);
/* or-ed into nwv_staged_run's mode: launch kernel by kernel with HIP events around each one
 * (feeds nwv_staged_kernel_times).  Untimed mode-1 runs replay a HIP graph of the batch MSM
 * captured on the batch's first untimed run. */
#define NWV_RUN_TIMED 0x100
int nwv_staged_sync(nwv_staged* st);
int nwv_staged_fetch(nwv_staged* st, uint64_t* verdict_bits, int* all_valid);
/* average device time (ms) per run of each pipeline kernel since the last reset, measured
 * with HIP events on the stream the kernels run on: avg_ms[0] = k_ed_hash (K1, K3),
 * avg_ms[1] = k_ed_points (K2), avg_ms[2] = k_ed_straus (K4, the dominant kernel) */
int nwv_staged_kernel_ms(nwv_staged* st, double avg_ms[3], int reset);
/* per-kernel average device time (ms) of mode `mode` runs since the last reset: fills up to
 * cap (name, ms) pairs in launch order (names point to static strings) and returns the number
 * of kernels in that pipeline (< 0 on error).  mode 1 (batch MSM, K5) kernels:
 * k_msm_prep (hash + decompression + the basepoint term), k_msm_hist, k_msm_wscan,
 * k_msm_scatter, k_msm_bucket, k_msm_tail; k_msm_keysum is timed with k_msm_prep, and
 * batches whose counting sort fits one chunk per window time k_msm_sort1 as k_msm_hist with
 * zero-length k_msm_wscan / k_msm_scatter slots.  Under NWV_FLAG_MSM_SPLIT_PREP k_msm_prep is
 * split into k_msm_scalars and k_msm_points. */
int nwv_staged_kernel_times(nwv_staged* st, int mode, int cap, const char** names, double* avg_ms,
                            int reset);
/* shape of the staged batch's MSM (diagnostics for roofline accounting): out[0] points
 * (na + 1 + n), [1] windows, [2] windows that carry the R_i points (the 128-bit z range),
 * [3] buckets over all windows, [4] bucket entries of the last mode-1 run (0 before one),
 * [5] sort chunks, [6] entries per k_msm_bucket lane, [7] A points (n, or the distinct keys) */
int nwv_staged_msm_stats(nwv_staged* st, uint64_t out[8]);
/* batch verdicts of every mode-1 run since staging, counted on the device by the run itself
 * (graph replays included): out[0] accepted runs, out[1] rejected runs.  Waits for the stream. */
int nwv_staged_run_tally(nwv_staged* st, uint64_t out[2]);
/* step-completion timestamps: record HIP event `slot` (< 65536) on the batch's stream (it fires
 * when the work queued before it on that stream is done); *ms = time from a's mark to b's */
int nwv_staged_mark(nwv_staged* st, int slot);
int nwv_staged_mark_elapsed(nwv_staged* a, int slot_a, nwv_staged* b, int slot_b, float* ms);
void nwv_staged_free(nwv_staged* st);

/* ------------------------------------------------------------------ synthetic data ----- */
/* RFC 8032 key generation and signing on the GPU, for synthetic workloads and tests
 * (the reference signs on the CPU with SignatureService; this is tooling, not the verify
 * path).  seeds n x 32, msgs as above; outputs pk n x 32, sig n x 64. */
int nwv_ed25519_sign_many(nwv_ctx* ctx, size_t n, const uint8_t* seeds, const uint8_t* msg_base,
                          const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* pk_out,
                          uint8_t* sig_out);

#ifdef __cplusplus
}
#endif
#endif /* NWV_H */
