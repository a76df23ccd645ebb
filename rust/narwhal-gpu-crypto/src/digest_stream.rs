//! The digest stream (`include/nwv_digest_stream.h`): BLAKE2b-256 digests of worker batches for a
//! caller that hashes them one at a time as they arrive, as the worker's `Processor` does
//! (`worker/src/processor.rs:38-71`: `serialized_batch_digest`, then the store write).
//!
//! `serialized_batch_digests` (lib.rs) blocks for a batch's whole chain of compressions and holds
//! one of the device's lanes.  A stream takes a batch, copies it and returns; the GPU hashes every
//! batch in flight in short slices and the digest arrives through `PendingDigest::wait`:
//!
//! ```ignore
//! let ds = DigestStream::open(-1, 0, 0, 0)?;                  // least-loaded device, defaults
//! // Processor::spawn: `while let Some(batch) = rx_batch.recv().await`
//! let pending = ds.submit_serialized(&batch)?;                 // returns at once
//! store.write(...);                                            // overlap whatever does not need the digest
//! let digest = tokio::task::spawn_blocking(move || pending.wait()).await??;
//! ```
//!
//! INTEGRATION.md says when the host's own `blake2b_256` is the better choice.
use std::os::raw::c_void;
use std::sync::mpsc::{sync_channel, Receiver, SyncSender};

use crate::{ctx, ffi, last_error};

/// Where the library writes a message's digest and error offset, and how its callback reports
/// back.  Boxed: its address is the callback's `user` word until the callback has fired.
struct Slot {
    digest: [u8; 32],
    err_offset: i64,
    tx: SyncSender<i32>,
}

unsafe extern "C" fn on_done(user: *mut c_void, result: i32) {
    let slot = &*(user as *const Slot);
    let _ = slot.tx.send(result);
}

/// Why a message has no digest.
#[derive(Debug, Clone, PartialEq, Eq)]
pub enum DigestFailure {
    /// `DigestError::InvalidArgumentError(offset)`: the bincode field at `offset` could not be read
    Malformed(i64),
    /// a negative engine code (a failed launch, or the stream was closed under the message)
    Engine(i32),
}

/// One submitted message.  Dropping it waits for the callback (the library holds its address).
pub struct PendingDigest {
    slot: Box<Slot>,
    rx: Receiver<i32>,
    fired: bool,
}
unsafe impl Send for PendingDigest {}

impl PendingDigest {
    fn new() -> Self {
        let (tx, rx) = sync_channel(1);
        PendingDigest { slot: Box::new(Slot { digest: [0u8; 32], err_offset: -1, tx }), rx, fired: false }
    }
    fn user(&mut self) -> *mut c_void {
        &mut *self.slot as *mut Slot as *mut c_void
    }
    /// Blocks until the message has completed.
    pub fn wait(mut self) -> Result<[u8; 32], DigestFailure> {
        let rc = self.rx.recv().unwrap_or(ffi::NWV_ERR_ARG);
        self.fired = true;
        if rc == ffi::NWV_OK {
            Ok(self.slot.digest)
        } else if self.slot.err_offset >= 0 {
            Err(DigestFailure::Malformed(self.slot.err_offset))
        } else {
            Err(DigestFailure::Engine(rc))
        }
    }
}

impl Drop for PendingDigest {
    fn drop(&mut self) {
        if !self.fired {
            let _ = self.rx.recv();
        }
    }
}

/// A message hashed while it is still being assembled or received.
pub struct PiecewiseDigest<'a> {
    stream: &'a DigestStream,
    id: u64,
    pending: Option<PendingDigest>,
}

impl<'a> PiecewiseDigest<'a> {
    pub fn update(&mut self, data: &[u8]) -> Result<(), String> {
        let rc = unsafe { ffi::nwv_dstream_update(ctx(), self.stream.id, self.id, data.as_ptr(), data.len()) };
        DigestStream::ok(rc)
    }
    pub fn finish(mut self) -> Result<PendingDigest, String> {
        let rc = unsafe { ffi::nwv_dstream_finish(ctx(), self.stream.id, self.id) };
        match self.pending.take() {
            Some(p) if rc == ffi::NWV_OK => Ok(p),
            p => {
                self.pending = p; // (dropped below: finished again, or left to the stream's close)
                Err(last_error())
            }
        }
    }
}

impl<'a> Drop for PiecewiseDigest<'a> {
    /// A message abandoned before `finish` is finished here and its digest discarded, so that its
    /// callback fires and the slot goes back to the stream.
    fn drop(&mut self) {
        if let Some(mut p) = self.pending.take() {
            let rc = unsafe { ffi::nwv_dstream_finish(ctx(), self.stream.id, self.id) };
            if rc != ffi::NWV_OK {
                // the stream no longer knows the message: no callback is outstanding to wait for
                p.fired = true;
            }
        }
    }
}

/// Counters of `nwv_dstream_stats`.
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct DigestStreamStats {
    pub messages: u64,
    pub ticks: u64,
    pub compressions: u64,
    pub uploaded: u64,
    pub tick_messages: u64,
    pub chunks: u64,
    pub chunks_peak: u64,
    pub waited: u64,
}

pub struct DigestStream {
    id: i32,
}

impl DigestStream {
    fn ok(rc: i32) -> Result<(), String> {
        if rc == ffi::NWV_OK {
            Ok(())
        } else {
            Err(last_error())
        }
    }
    /// `device_index` -1: the least-loaded device; 0 for a size: the library's default.
    pub fn open(device_index: i32, slice_blocks: usize, pool_chunks: usize, max_messages: usize) -> Result<Self, String> {
        let id = unsafe { ffi::nwv_dstream_open(ctx(), device_index, slice_blocks, pool_chunks, max_messages) };
        if id >= 0 {
            Ok(DigestStream { id })
        } else {
            Err(last_error())
        }
    }
    /// `Batch::digest` of the concatenated transaction bytes (types/src/primary.rs:65-73).
    pub fn submit(&self, data: &[u8]) -> Result<PendingDigest, String> {
        let mut p = PendingDigest::new();
        let user = p.user();
        let rc = unsafe {
            ffi::nwv_dstream_submit(ctx(), self.id, data.as_ptr(), data.len(), p.slot.digest.as_mut_ptr(), Some(on_done), user)
        };
        if rc != ffi::NWV_OK {
            p.fired = true; // no callback fires for a refused submission
        }
        Self::ok(rc).map(|_| p)
    }
    /// `serialized_batch_digest` (types/src/worker.rs:44-62) of one bincode `WorkerMessage::Batch`.
    pub fn submit_serialized(&self, buf: &[u8]) -> Result<PendingDigest, String> {
        let mut p = PendingDigest::new();
        let user = p.user();
        let rc = unsafe {
            ffi::nwv_dstream_submit_serialized(
                ctx(), self.id, buf.as_ptr(), buf.len(), p.slot.digest.as_mut_ptr(), &mut p.slot.err_offset, Some(on_done),
                user,
            )
        };
        if rc != ffi::NWV_OK {
            p.fired = true;
        }
        Self::ok(rc).map(|_| p)
    }
    pub fn begin(&self) -> Result<PiecewiseDigest<'_>, String> {
        let mut p = PendingDigest::new();
        let user = p.user();
        let mut id = 0u64;
        let rc = unsafe { ffi::nwv_dstream_begin(ctx(), self.id, p.slot.digest.as_mut_ptr(), Some(on_done), user, &mut id) };
        if rc != ffi::NWV_OK {
            p.fired = true;
        }
        Self::ok(rc).map(|_| PiecewiseDigest { stream: self, id, pending: Some(p) })
    }
    /// Returns once everything submitted or finished before the call has completed.
    pub fn flush(&self) -> Result<(), String> {
        Self::ok(unsafe { ffi::nwv_dstream_flush(ctx(), self.id) })
    }
    pub fn stats(&self) -> DigestStreamStats {
        let mut o = [0u64; 8];
        unsafe { ffi::nwv_dstream_stats(ctx(), self.id, o.as_mut_ptr()) };
        DigestStreamStats {
            messages: o[0],
            ticks: o[1],
            compressions: o[2],
            uploaded: o[3],
            tick_messages: o[4],
            chunks: o[5],
            chunks_peak: o[6],
            waited: o[7],
        }
    }
}

impl Drop for DigestStream {
    /// Finished messages complete; a `PiecewiseDigest` never finished completes with `NWV_ERR_ARG`.
    fn drop(&mut self) {
        unsafe {
            ffi::nwv_dstream_close(ctx(), self.id);
        }
    }
}
