/*
 * nwv_digest_stream.h -- streaming BLAKE2b-256 digests of worker batches (SURVEY.md §8 a5, a6, a15,
 * f2): Batch::digest (types/src/primary.rs:65-73) and serialized_batch_digest
 * (types/src/worker.rs:44-80) for a caller that hashes batches as they arrive
 * (worker/src/processor.rs:38-71).
 *
 * nwv_blake2b256_many and nwv_batch_digest_serialized block their caller, hold one of a device's
 * lanes for a ~500 KB batch's whole chain of 3,909 compressions and copy every byte before the
 * first one.  A digest stream takes any number of messages, whole or piecewise, from any number of
 * threads; a pump thread hashes them in ticks of at most slice_blocks compressions a message
 * (k_blake2b_slice: the chaining value is kept per message between launches), uploads the next
 * tick's bytes under the current tick's kernel and completes each message by callback.  A stream
 * takes no lane from the lane pools: verification and the one-call digests never wait for it.
 *
 * A stream is a small integer owned by the context (at most 8 open at a time; nwv_free closes
 * them).  Messages are copied at submission: the caller's buffer is free again when the call
 * returns.  digest_out (32 bytes) stays the caller's and is written before done(user, result)
 * fires; result is NWV_OK, or the negative error of a failed launch.  done fires exactly once per
 * accepted message, on the stream's thread, with no lock held; it may be null.  From inside a
 * callback, a call that would have to wait for pool space, nwv_dstream_flush and
 * nwv_dstream_close return NWV_ERR_REENTRANT.  All entry points are thread-safe; the updates of
 * one message are the caller's to order.
 */
#ifndef NWV_DIGEST_STREAM_H
#define NWV_DIGEST_STREAM_H

#include <stddef.h>
#include <stdint.h>

#include "nwv.h"
#include "nwv_service.h"

#ifdef __cplusplus
extern "C" {
#endif

/* returns a stream id >= 0 or a negative error; device_index -1 = least-loaded device;
 * slice_blocks 0 / pool_chunks 0 / max_messages 0 = defaults (1,024 compressions a tick and message,
 * a 64 MiB pool, 128 messages in flight).  The pool is pool_chunks chunks of slice_blocks x 128
 * bytes, in pinned host memory and on the device; pool_chunks >= 2 max_messages is required. */
int nwv_dstream_open(nwv_ctx* ctx, int device_index, size_t slice_blocks, size_t pool_chunks, size_t max_messages);
/* whole message (the Batch::digest stream); waits for a message slot and pool space */
int nwv_dstream_submit(nwv_ctx* ctx, int ds, const uint8_t* data, size_t len, uint8_t* digest_out, nwv_done_fn done,
                       void* user);
/* bincode WorkerMessage::Batch: only the transaction bytes are hashed.  Malformed: the call still
 * returns NWV_OK, done fires with NWV_ERR_ARG and *err_offset_out holds the offset of the field that
 * could not be read (else -1; written before the call returns), as nwv_batch_digest_serialized */
int nwv_dstream_submit_serialized(nwv_ctx* ctx, int ds, const uint8_t* buf, size_t len, uint8_t* digest_out,
                                  int64_t* err_offset_out, nwv_done_fn done, void* user);
/* piecewise: hash a message while it is still being assembled or received */
int nwv_dstream_begin(nwv_ctx* ctx, int ds, uint8_t* digest_out, nwv_done_fn done, void* user, uint64_t* msg_id);
int nwv_dstream_update(nwv_ctx* ctx, int ds, uint64_t msg_id, const uint8_t* data, size_t len);
int nwv_dstream_finish(nwv_ctx* ctx, int ds, uint64_t msg_id);
/* returns once everything submitted or finished before the call has completed */
int nwv_dstream_flush(nwv_ctx* ctx, int ds);
/* out[0] messages completed, [1] ticks launched, [2] compressions run, [3] bytes uploaded, [4] most
 * messages in one tick, [5] chunks in use, [6] peak chunks in use, [7] submissions that waited for
 * pool space or a message slot */
int nwv_dstream_stats(nwv_ctx* ctx, int ds, uint64_t out[8]);
/* completes finished messages; never-finished ones get done(user, NWV_ERR_ARG); the id is free again */
int nwv_dstream_close(nwv_ctx* ctx, int ds);

#ifdef __cplusplus
}
#endif
#endif /* NWV_DIGEST_STREAM_H */
