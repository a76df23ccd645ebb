"""Streaming BLAKE2b-256 digests of worker batches (include/nwv_digest_stream.h).

    with DigestStream(eng) as ds:
        p = ds.submit_serialized(buf)           # returns at once; the bytes are copied
        q = ds.submit(payload, callback=fn)     # fn(pending) runs on the stream's thread
        m = ds.begin(); m.update(part1); m.update(part2); m.finish()
        ds.flush()
        p.digest(), p.err_offset

A stream hashes every message in flight in ticks of at most slice_blocks compressions each on the
GPU (k_blake2b_slice), uploads under the running tick and completes each message by callback; it
leases no lane, so verification calls on the same Engine never wait for it.  The one-call forms
(Engine.blake2b256_many, Engine.batch_digest_serialized) stay what they were.
"""
import ctypes
import itertools
import threading

import numpy as np

from ._lib import NWV_ERR_ARG, NWV_OK, _check

STAT_NAMES = ("messages", "ticks", "compressions", "uploaded", "tick_messages", "chunks", "chunks_peak", "waited")
_DONE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int32)


class Pending:
    """One message of a stream: wait() -> result code, digest() -> 32 bytes (None when the message
    failed), err_offset (serialized submissions: -1, or the offset of the malformed field)."""

    def __init__(self, stream, callback):
        self._stream = stream
        self._callback = callback
        self._out = np.zeros(32, dtype=np.uint8)
        self._err = ctypes.c_int64(-1)
        self._event = threading.Event()
        self.result = None
        self.fired = 0  # times the completion callback ran (exactly once when all is well)
        self._id = None

    @property
    def err_offset(self):
        return int(self._err.value)

    def wait(self, timeout=None):
        if not self._event.wait(timeout):
            raise TimeoutError("digest stream: the message has not completed")
        return self.result

    def digest(self, timeout=None):
        return self._out.tobytes() if self.wait(timeout) == NWV_OK else None

    # piecewise messages (DigestStream.begin)
    def update(self, data):
        s = self._stream
        data = bytes(data)
        _check(s.lib.nwv_dstream_update(s.eng._h, s.id, self._id, data, len(data)))
        return self

    def finish(self):
        s = self._stream
        _check(s.lib.nwv_dstream_finish(s.eng._h, s.id, self._id))
        return self


class DigestStream:
    """nwv_dstream_open on an Engine: device_index -1 picks the least-loaded device; 0 for
    slice_blocks, pool_chunks or max_messages takes the library's default."""

    def __init__(self, eng, device_index=-1, slice_blocks=0, pool_chunks=0, max_messages=0):
        self.eng, self.lib = eng, eng.lib
        if not hasattr(self.lib, "nwv_dstream_open"):
            raise ImportError("this libnwv.so has no digest stream")
        self._pending = {}
        self._keys = itertools.count(1)
        self._mu = threading.Lock()
        self._trampoline = _DONE_FN(self._on_done)  # (kept alive with the stream)
        self.id = _check(self.lib.nwv_dstream_open(eng._h, int(device_index), int(slice_blocks), int(pool_chunks),
                                                   int(max_messages)), allow=range(0, 8))
        # the Engine keeps its open streams (and with them their callback trampolines) alive: closing
        # the Engine closes them in the library, which completes what is left by callback
        eng.__dict__.setdefault("_dstreams", set()).add(self)

    def _on_done(self, user, result):
        with self._mu:
            p = self._pending.pop(user, None)
        if p is None:
            return
        p.result = int(result)
        p.fired += 1
        try:
            if p._callback is not None:
                p._callback(p)
        finally:
            p._event.set()

    def _register(self, callback):
        p = Pending(self, callback)
        key = next(self._keys)
        with self._mu:
            self._pending[key] = p
        return p, key

    def _drop(self, key):
        with self._mu:
            self._pending.pop(key, None)

    def submit(self, data, callback=None):
        """a whole message (the Batch::digest stream); waits for pool space -> Pending"""
        data = bytes(data)
        p, key = self._register(callback)
        rc = self.lib.nwv_dstream_submit(self.eng._h, self.id, data, len(data), p._out.ctypes.data, self._trampoline,
                                         key)
        if rc != NWV_OK:
            self._drop(key)
            _check(rc)
        return p

    def submit_serialized(self, buf, callback=None):
        """a bincode WorkerMessage::Batch; a malformed one completes with NWV_ERR_ARG and err_offset set"""
        buf = bytes(buf)
        p, key = self._register(callback)
        rc = self.lib.nwv_dstream_submit_serialized(self.eng._h, self.id, buf, len(buf), p._out.ctypes.data,
                                                    ctypes.byref(p._err), self._trampoline, key)
        if rc != NWV_OK:
            self._drop(key)
            _check(rc)
        return p

    def begin(self, callback=None):
        """a message hashed while it is assembled: Pending.update(bytes)..., Pending.finish()"""
        p, key = self._register(callback)
        mid = ctypes.c_uint64(0)
        rc = self.lib.nwv_dstream_begin(self.eng._h, self.id, p._out.ctypes.data, self._trampoline, key,
                                        ctypes.byref(mid))
        if rc != NWV_OK:
            self._drop(key)
            _check(rc)
        p._id = mid.value
        return p

    def flush(self):
        """returns once everything submitted or finished before the call has completed"""
        _check(self.lib.nwv_dstream_flush(self.eng._h, self.id))

    def stats(self):
        out = np.zeros(len(STAT_NAMES), dtype=np.uint64)
        _check(self.lib.nwv_dstream_stats(self.eng._h, self.id, out.ctypes.data))
        return {k: int(v) for k, v in zip(STAT_NAMES, out)}

    def close(self):
        """completes finished messages; never-finished ones complete with NWV_ERR_ARG"""
        if self.id is not None and self.eng._h:
            sid, self.id = self.id, None
            try:
                _check(self.lib.nwv_dstream_close(self.eng._h, sid))
            except Exception:
                self.id = sid
                raise
            self.eng.__dict__.get("_dstreams", set()).discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def digest_results(pendings):
    """[(digest or None, err_offset)] of serialized submissions, the shape of
    Engine.batch_digest_serialized"""
    out = []
    for p in pendings:
        rc = p.wait()
        if rc not in (NWV_OK, NWV_ERR_ARG):
            _check(rc)
        out.append((p._out.tobytes() if rc == NWV_OK else None, p.err_offset))
    return out
