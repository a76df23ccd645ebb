// digest_stream.h -- a streaming BLAKE2b-256 digest pipeline for worker batches (host code, no HIP).
//
// Batch::digest (types/src/primary.rs:65-73) and serialized_batch_digest (types/src/worker.rs:44-80)
// hash ~500 KB a batch: 3,909 dependent compressions.  The one-call forms (nwv_blake2b256_many,
// nwv_batch_digest_serialized) hold a lane for the whole chain and copy every byte before the first
// compression.  A digest stream instead accepts any number of messages, whole or piecewise, and
// hashes them in ticks: every tick runs at most slice_blocks compressions of every message that
// has blocks ready (k_blake2b_slice, resumable: the chaining value lives in a per-message slot),
// so a launch is short, uploads of the next tick run under the current tick's kernel, and a message
// completes by callback.
//
// This header is the whole stream except the device: the chunk pool, the hold-back rule, the tick
// plan, the bincode walk, the pump thread, backpressure and the callbacks.  The device is a
// DsBackend (the engine's: two HIP streams and k_blake2b_slice; the host tests': the same work
// records run with blake2b.h's compression, tests/hostemu/digest_stream_stub.cpp).
//
// Chunk pool.  pool_chunks chunks of slice_blocks x 128 bytes; a pinned host pool and the device
// pool share indices.  A message's k-th chunk holds its blocks [k S, (k + 1) S).  A chunk goes
// back to the free list when the tick that consumed its last block has completed.
//
// Hold-back rule (BLAKE2b's update rule: the last block is compressed with the final flag, so it
// is not known to be a middle block until a byte follows it).  An unfinished message of L bytes
// has floor((L - 1) / 128) releasable blocks (none for L = 0): never its last buffered block, even
// a full one.  finish releases the rest; the last block carries last_len = L - 128 (nb - 1), an
// empty message is one zero block with last_len 0, and a message of exactly k 128 bytes ends on
// its k-th block.
//
// Only the current write chunk of a message can hold blocks that no tick may consume yet, so at
// most max_messages chunks are ever unconsumable; pool_chunks >= 2 max_messages (required) leaves
// chunks that the pump frees, and a message larger than the whole pool goes through.
//
// One mutex guards slots, chunks and counters.  Callbacks fire on the pump thread with the mutex
// released; from inside one, a call that would have to wait (and flush, and close) returns
// DS_ERR_REENTRANT.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

namespace nwv {

// the values of NWV_OK, NWV_ERR_ARG and NWV_ERR_REENTRANT (include/nwv.h)
constexpr int DS_OK = 0, DS_ERR_ARG = -1, DS_ERR_REENTRANT = -7;
constexpr uint32_t DS_FIRST = 1, DS_LAST = 2;
constexpr size_t DS_BLOCK = 128;
constexpr size_t DS_MAX_MESSAGES = 65536;  // a message id carries its slot in 16 bits

// One record per active message per tick (32 bytes; k_blake2b_slice reads it as two uint4):
// run nblocks compressions from block first_block of pool chunk `chunk`, on the state of `slot`.
struct DsRecord {
    uint32_t slot, chunk, first_block, nblocks;
    uint32_t flags, last_len, pad0, pad1;
};
static_assert(sizeof(DsRecord) == 32, "k_blake2b_slice's record layout");

struct DsCopy {
    uint64_t off, len;  // bytes of the pool (the same range of the host and the device pool)
};

typedef void (*ds_done_fn)(void* user, int32_t result);

struct DsDone {
    uint32_t slot;
    uint8_t* digest_out;
    ds_done_fn done;
    void* user;
    int32_t result;
    uint64_t seq;
};

struct DsTick {
    std::vector<DsRecord> recs;    // by nblocks, longest first (a wave's trip count is its maximum)
    std::vector<DsCopy> copies;    // every block the records read, adjacent ranges merged
    std::vector<uint32_t> chunks;  // chunks whose last block this tick consumes
    std::vector<DsDone> done;      // messages whose last block this tick compresses
    void clear() {
        recs.clear();
        copies.clear();
        chunks.clear();
        done.clear();
    }
};

// The device of a stream.  submit and wait are called by the pump thread only, without the
// stream's mutex; at most two ticks (buf 0 and 1) are between submit and wait.
struct DsBackend {
    virtual ~DsBackend() {}
    virtual uint8_t* host_pool() = 0;
    // upload the tick's copies, then run its records (asynchronously)
    virtual int submit(int buf, const DsTick& t) = 0;
    // returns once that tick has completed; the digests of its DS_LAST records are then readable
    virtual int wait(int buf) = 0;
    virtual const uint8_t* digests() = 0;  // 32 bytes a slot
    // the stream has (on) or no longer has messages in flight
    virtual void busy(bool on) { (void)on; }
};

// 1 while the calling thread runs a completion callback of any stream
inline int& ds_in_callback() {
    static thread_local int v = 0;
    return v;
}

// Walk of a bincode WorkerMessage::Batch buffer ([u32 variant][u64 count][(u64 len, bytes)]*,
// types/src/worker.rs:44-80) as k_batch_compact walks it: the transaction byte ranges in order, or
// the offset of the u64 field that could not be read.  Returns -1 when the buffer is well formed.
struct DsSeg {
    const uint8_t* p;
    size_t len;
};
inline uint64_t ds_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
    return v;
}
inline int64_t ds_walk_batch(const uint8_t* buf, size_t L, std::vector<DsSeg>& segs) {
    segs.clear();
    if (L < 12) return 4;
    uint64_t left = ds_le64(buf + 4), pos = 12;
    while (left > 0) {
        if (pos + 8 > L) return (int64_t)pos;
        const uint64_t tl = ds_le64(buf + pos);
        if (tl > L - pos - 8) return (int64_t)pos;
        if (tl) segs.push_back(DsSeg{buf + pos + 8, (size_t)tl});
        pos += 8 + tl;
        left--;
    }
    return -1;
}

enum {
    DS_STAT_MESSAGES = 0,   // messages completed
    DS_STAT_TICKS,          // ticks launched
    DS_STAT_COMPRESSIONS,   // compressions run
    DS_STAT_UPLOADED,       // bytes uploaded
    DS_STAT_TICK_MESSAGES,  // most messages in one tick
    DS_STAT_CHUNKS,         // chunks in use
    DS_STAT_CHUNKS_PEAK,    // peak chunks in use
    DS_STAT_WAITED,         // submissions that waited for pool space
    DS_STATS
};

class DigestStream {
  public:
    // defaults: 1,024 blocks a slice (the smallest swept slice whose round rate was within the spread
    // of the best), 128 messages, a 64 MiB pool (and at least 2 max_messages chunks)
    static size_t default_slice() { return 1024; }
    static size_t default_messages() { return 128; }
    static size_t default_chunks(size_t slice, size_t messages) {
        return std::max<size_t>(2 * messages, ((size_t)64 << 20) / (slice * DS_BLOCK));
    }
    static bool config_ok(size_t slice, size_t chunks, size_t messages) {
        return slice >= 1 && slice <= ((size_t)1 << 20) && messages >= 1 && messages <= DS_MAX_MESSAGES &&
               chunks >= 2 * messages && chunks <= ((size_t)1 << 24);
    }

    // the backend's pools hold `chunks` chunks of slice x 128 bytes and its state `messages` slots
    DigestStream(DsBackend& be, size_t slice, size_t chunks, size_t messages)
        : be_(be), S_(slice), CB_(slice * DS_BLOCK), slots_(messages) {
        for (size_t c = chunks; c-- > 0;) free_chunks_.push_back((uint32_t)c);
        for (size_t s = messages; s-- > 0;) free_slots_.push_back((uint32_t)s);
        pump_ = std::thread([this] { pump(); });
    }
    ~DigestStream() { (void)close(); }
    DigestStream(const DigestStream&) = delete;
    DigestStream& operator=(const DigestStream&) = delete;

    int begin(uint8_t* digest_out, ds_done_fn done, void* user, uint64_t* msg_id) {
        if (!digest_out || !msg_id) return DS_ERR_ARG;
        std::unique_lock<std::mutex> lk(mu_);
        Call call(*this);
        if (!call.ok) return DS_ERR_ARG;
        uint32_t slot;
        const int rc = take_slot(lk, slot, digest_out, done, user, false);
        if (rc) return rc;
        *msg_id = slots_[slot].id;
        return DS_OK;
    }

    int update(uint64_t msg_id, const uint8_t* data, size_t len) {
        if (len && !data) return DS_ERR_ARG;
        std::unique_lock<std::mutex> lk(mu_);
        Call call(*this);
        if (!call.ok) return DS_ERR_ARG;
        Msg* m = find(msg_id);
        if (!m) return DS_ERR_ARG;
        const DsSeg seg{data, len};
        m->busy = true;
        const int rc = append(lk, *m, &seg, 1);
        m->busy = false;
        return rc;
    }

    int finish(uint64_t msg_id) {
        std::unique_lock<std::mutex> lk(mu_);
        Call call(*this);
        if (!call.ok) return DS_ERR_ARG;
        Msg* m = find(msg_id);
        if (!m) return DS_ERR_ARG;
        m->busy = true;
        const int rc = finish_locked(lk, *m);
        m->busy = false;
        return rc;
    }

    // a whole message: begin, update, finish.  When it fails, no callback fires.
    int submit(const uint8_t* data, size_t len, uint8_t* digest_out, ds_done_fn done, void* user) {
        const DsSeg seg{data, len};
        if (len && !data) return DS_ERR_ARG;
        return submit_segs(&seg, 1, len, 0, digest_out, done, user);
    }

    // a bincode WorkerMessage::Batch: only the transaction bytes are hashed.  A malformed buffer is
    // accepted too: its callback fires with DS_ERR_ARG, *err_offset_out holds the offset of the field
    // that could not be read, and digest_out the digest of no bytes (as nwv_batch_digest_serialized).
    int submit_serialized(const uint8_t* buf, size_t len, uint8_t* digest_out, int64_t* err_offset_out,
                          ds_done_fn done, void* user) {
        if (!buf || !err_offset_out) return DS_ERR_ARG;
        std::vector<DsSeg> segs;
        const int64_t err = ds_walk_batch(buf, len, segs);
        *err_offset_out = err;
        if (err >= 0) return submit_segs(nullptr, 0, 0, DS_ERR_ARG, digest_out, done, user);
        size_t total = 0;
        for (const DsSeg& s : segs) total += s.len;
        return submit_segs(segs.data(), segs.size(), total, 0, digest_out, done, user);
    }

    // returns once every message submitted or finished before the call has completed
    int flush() {
        if (ds_in_callback()) return DS_ERR_REENTRANT;
        std::unique_lock<std::mutex> lk(mu_);
        Call call(*this);
        if (!call.ok) return DS_ERR_ARG;
        const uint64_t upto = next_seq_;
        done_cv_.wait(lk, [&] { return open_.empty() || *open_.begin() >= upto; });
        return DS_OK;
    }

    void stats(uint64_t out[DS_STATS]) {
        std::lock_guard<std::mutex> g(mu_);
        std::memcpy(out, stat_, sizeof stat_);
    }

    // completes every finished message, stops the pump, then fails every never-finished message
    // with DS_ERR_ARG.  Calls that arrive afterwards return DS_ERR_ARG.
    int close() {
        if (ds_in_callback()) return DS_ERR_REENTRANT;
        std::vector<DsDone> orphans;
        {
            std::unique_lock<std::mutex> lk(mu_);
            if (closing_) return DS_ERR_ARG;
            closing_ = true;
            space_cv_.notify_all();
            done_cv_.wait(lk, [&] { return calls_ == 0; });
            done_cv_.wait(lk, [&] { return open_.empty(); });
            stop_ = true;
            pump_cv_.notify_all();
        }
        pump_.join();
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t s = 0; s < slots_.size(); s++) {
                Msg& m = slots_[s];
                if (!m.live) continue;
                if (!m.whole) orphans.push_back(DsDone{(uint32_t)s, m.digest_out, m.done, m.user, DS_ERR_ARG, 0});
                release_chunks(m);
                m.live = false;
                live_--;
            }
            if (busy_) be_.busy(false);
            busy_ = false;
        }
        ds_in_callback()++;
        for (const DsDone& d : orphans)
            if (d.done) d.done(d.user, d.result);
        ds_in_callback()--;
        return DS_OK;
    }

  private:
    struct Msg {
        bool live = false, finished = false, closing = false, busy = false;
        bool whole = false;    // begun by submit: no callback unless its submit succeeds
        bool aborted = false;  // its submit failed: no tick takes it any more
        uint64_t id = 0;
        uint8_t* digest_out = nullptr;
        ds_done_fn done = nullptr;
        void* user = nullptr;
        int32_t result = 0;
        uint64_t len = 0;      // bytes published
        uint64_t planned = 0;  // blocks handed to ticks
        uint64_t seq = 0;      // order of finish
        uint64_t chunk0 = 0;   // chunks[j] is the message's chunk chunk0 + j
        std::deque<uint32_t> chunks;
    };
    // a call in progress (close waits for them); constructed and destroyed under the mutex
    struct Call {
        DigestStream& s;
        bool ok;
        explicit Call(DigestStream& st) : s(st), ok(!st.closing_) {
            if (ok) s.calls_++;
        }
        ~Call() {
            if (ok && --s.calls_ == 0) s.done_cv_.notify_all();
        }
    };

    uint64_t total_blocks(const Msg& m) const { return m.len == 0 ? 1 : (m.len + DS_BLOCK - 1) / DS_BLOCK; }
    uint64_t releasable(const Msg& m) const {
        if (m.finished) return total_blocks(m);
        return m.len == 0 ? 0 : (m.len - 1) / DS_BLOCK;
    }
    Msg* find(uint64_t id) {
        Msg& m = slots_[(size_t)(id & 0xffff) % slots_.size()];
        return (m.live && m.id == id && !m.finished && !m.busy && !m.aborted) ? &m : nullptr;
    }
    void release_chunks(Msg& m) {
        for (uint32_t c : m.chunks) free_chunk(c);
        m.chunks.clear();
    }
    void free_chunk(uint32_t c) {
        free_chunks_.push_back(c);
        stat_[DS_STAT_CHUNKS]--;
    }
    uint32_t take_chunk() {
        const uint32_t c = free_chunks_.back();
        free_chunks_.pop_back();
        if (++stat_[DS_STAT_CHUNKS] > stat_[DS_STAT_CHUNKS_PEAK]) stat_[DS_STAT_CHUNKS_PEAK] = stat_[DS_STAT_CHUNKS];
        return c;
    }
    // wait (under lk) until pred holds; DS_ERR_REENTRANT from a callback, DS_ERR_ARG once closing
    template <class Pred>
    int wait_space(std::unique_lock<std::mutex>& lk, Pred pred) {
        if (pred()) return closing_ ? DS_ERR_ARG : DS_OK;
        if (ds_in_callback()) return DS_ERR_REENTRANT;
        stat_[DS_STAT_WAITED]++;
        space_cv_.wait(lk, [&] { return closing_ || pred(); });
        return closing_ ? DS_ERR_ARG : DS_OK;
    }

    int take_slot(std::unique_lock<std::mutex>& lk, uint32_t& slot, uint8_t* digest_out, ds_done_fn done, void* user,
                  bool whole) {
        const int rc = wait_space(lk, [&] { return !free_slots_.empty(); });
        if (rc) return rc;
        slot = free_slots_.back();
        free_slots_.pop_back();
        Msg& m = slots_[slot];
        m = Msg();
        m.live = true;
        m.id = (++serial_ << 16) | slot;
        m.digest_out = digest_out;
        m.done = done;
        m.user = user;
        m.whole = whole;
        if (live_++ == 0 && !busy_) {
            busy_ = true;
            be_.busy(true);
        }
        return DS_OK;
    }

    // chunks that `add` more bytes of m need beyond those it holds
    size_t chunks_needed(const Msg& m, uint64_t add) const {
        const uint64_t end = m.len + add;
        const uint64_t have = m.chunk0 + m.chunks.size();
        const uint64_t want = (end + CB_ - 1) / CB_;
        return want > have ? (size_t)(want - have) : 0;
    }

    int append(std::unique_lock<std::mutex>& lk, Msg& m, const DsSeg* segs, size_t nseg) {
        uint64_t total = 0;
        for (size_t i = 0; i < nseg; i++) total += segs[i].len;
        if (ds_in_callback()) {
            // the pump is the caller: nothing frees while it is here, so the chunks are taken at once
            const size_t need = chunks_needed(m, total);
            if (need > free_chunks_.size()) return DS_ERR_REENTRANT;
            for (size_t k = 0; k < need; k++) m.chunks.push_back(take_chunk());
        }
        size_t si = 0, so = 0;
        while (si < nseg) {
            if (segs[si].len == so) {
                si++;
                so = 0;
                continue;
            }
            const uint64_t pos = m.len, k = pos / CB_, o = pos % CB_;
            if (k - m.chunk0 >= m.chunks.size()) {
                const int rc = wait_space(lk, [&] { return !free_chunks_.empty(); });
                if (rc) return rc;
                m.chunks.push_back(take_chunk());
            }
            uint8_t* dst = be_.host_pool() + (size_t)m.chunks[(size_t)(k - m.chunk0)] * CB_ + o;
            size_t space = (size_t)(CB_ - o), wrote = 0;
            // the bytes past m.len belong to this call alone (no tick reads an unpublished block)
            lk.unlock();
            while (space && si < nseg) {
                const size_t n = std::min(space, segs[si].len - so);
                std::memcpy(dst + wrote, segs[si].p + so, n);
                wrote += n;
                space -= n;
                so += n;
                if (so == segs[si].len) {
                    si++;
                    so = 0;
                }
            }
            lk.lock();
            m.len += wrote;
            if (releasable(m) > m.planned) pump_cv_.notify_one();
        }
        return DS_OK;
    }

    int finish_locked(std::unique_lock<std::mutex>& lk, Msg& m) {
        if (m.len == 0 && m.chunks.empty()) {
            const int rc = wait_space(lk, [&] { return !free_chunks_.empty(); });
            if (rc) return rc;
            m.chunks.push_back(take_chunk());
        }
        // the host zero-pads the final block
        const uint64_t nb = total_blocks(m), end = nb * DS_BLOCK;
        if (end > m.len) {
            const uint64_t k = m.len / CB_, o = m.len % CB_;
            std::memset(be_.host_pool() + (size_t)m.chunks[(size_t)(k - m.chunk0)] * CB_ + o, 0, (size_t)(end - m.len));
        }
        m.finished = true;
        m.whole = false;
        m.seq = next_seq_++;
        open_.insert(m.seq);
        pump_cv_.notify_one();
        return DS_OK;
    }

    int submit_segs(const DsSeg* segs, size_t nseg, size_t total, int32_t result, uint8_t* digest_out,
                    ds_done_fn done, void* user) {
        if (!digest_out) return DS_ERR_ARG;
        std::unique_lock<std::mutex> lk(mu_);
        Call call(*this);
        if (!call.ok) return DS_ERR_ARG;
        if (ds_in_callback() &&
            (free_slots_.empty() || std::max<size_t>(1, (total + CB_ - 1) / CB_) > free_chunks_.size()))
            return DS_ERR_REENTRANT;
        uint32_t slot;
        int rc = take_slot(lk, slot, digest_out, done, user, true);
        if (rc) return rc;
        Msg& m = slots_[slot];
        m.result = result;
        m.busy = true;
        rc = append(lk, m, segs, nseg);
        if (!rc) rc = finish_locked(lk, m);
        m.busy = false;
        if (rc) m.aborted = true;  // (close releases it, with no callback)
        return rc;
    }

    // One tick: at most one record a message, from its first unplanned block to the end of that
    // block's chunk or of what the hold-back rule releases.  Under the mutex.
    bool plan(DsTick& t) {
        t.clear();
        uint64_t blocks = 0;
        for (size_t s = 0; s < slots_.size(); s++) {
            Msg& m = slots_[s];
            if (!m.live || m.closing || m.aborted) continue;
            const uint64_t rel = releasable(m);
            if (m.planned >= rel) continue;
            const uint64_t k = m.planned / S_, fb = m.planned % S_;
            const uint64_t nbk = std::min<uint64_t>(rel - m.planned, S_ - fb);
            const uint32_t c = m.chunks[(size_t)(k - m.chunk0)];
            const bool last = m.finished && m.planned + nbk == rel;
            DsRecord r{};
            r.slot = (uint32_t)s;
            r.chunk = c;
            r.first_block = (uint32_t)fb;
            r.nblocks = (uint32_t)nbk;
            r.flags = (m.planned == 0 ? DS_FIRST : 0) | (last ? DS_LAST : 0);
            r.last_len = last ? (uint32_t)(m.len - DS_BLOCK * (rel - 1)) : 0;
            t.recs.push_back(r);
            t.copies.push_back(DsCopy{(uint64_t)c * CB_ + fb * DS_BLOCK, nbk * DS_BLOCK});
            m.planned += nbk;
            blocks += nbk;
            if (fb + nbk == S_ || last) {
                t.chunks.push_back(c);
                m.chunks.pop_front();
                m.chunk0++;
            }
            if (last) {
                for (uint32_t x : m.chunks) t.chunks.push_back(x);  // (none: a message holds what it wrote)
                m.chunks.clear();
                m.closing = true;
                t.done.push_back(DsDone{(uint32_t)s, m.digest_out, m.done, m.user, m.result, m.seq});
            }
        }
        if (t.recs.empty()) return false;
        std::stable_sort(t.recs.begin(), t.recs.end(),
                         [](const DsRecord& a, const DsRecord& b) { return a.nblocks > b.nblocks; });
        std::sort(t.copies.begin(), t.copies.end(), [](const DsCopy& a, const DsCopy& b) { return a.off < b.off; });
        size_t w = 0;
        for (size_t i = 1; i < t.copies.size(); i++) {
            if (t.copies[w].off + t.copies[w].len == t.copies[i].off)
                t.copies[w].len += t.copies[i].len;
            else
                t.copies[++w] = t.copies[i];
        }
        t.copies.resize(w + 1);
        stat_[DS_STAT_TICKS]++;
        stat_[DS_STAT_COMPRESSIONS] += blocks;
        stat_[DS_STAT_UPLOADED] += blocks * DS_BLOCK;
        stat_[DS_STAT_TICK_MESSAGES] = std::max<uint64_t>(stat_[DS_STAT_TICK_MESSAGES], t.recs.size());
        return true;
    }

    // Two ticks are kept in flight: tick n + 1 is planned and submitted (its upload runs under tick
    // n's kernel) before tick n is waited for.
    void pump() {
        std::unique_lock<std::mutex> lk(mu_);
        std::deque<int> inflight;
        int next = 0, broken = 0;
        for (;;) {
            if (inflight.size() < 2 && plan(tick_[next])) {
                lk.unlock();
                if (!broken) broken = be_.submit(next, tick_[next]);
                lk.lock();
                inflight.push_back(next);
                next ^= 1;
                continue;
            }
            if (!inflight.empty()) {
                const int b = inflight.front();
                inflight.pop_front();
                DsTick& t = tick_[b];
                lk.unlock();
                if (!broken) broken = be_.wait(b);
                ds_in_callback()++;
                for (const DsDone& d : t.done) {
                    const int32_t res = broken ? (int32_t)broken : d.result;
                    if (!broken) std::memcpy(d.digest_out, be_.digests() + 32 * (size_t)d.slot, 32);
                    if (d.done) d.done(d.user, res);
                }
                ds_in_callback()--;
                lk.lock();
                for (uint32_t c : t.chunks) free_chunk(c);
                for (const DsDone& d : t.done) {
                    slots_[d.slot].live = false;
                    free_slots_.push_back(d.slot);
                    open_.erase(d.seq);
                    stat_[DS_STAT_MESSAGES]++;
                    live_--;
                }
                if (live_ == 0 && busy_) {
                    busy_ = false;
                    be_.busy(false);
                }
                space_cv_.notify_all();
                done_cv_.notify_all();
                continue;
            }
            if (stop_) break;
            pump_cv_.wait(lk);
        }
    }

    DsBackend& be_;
    const size_t S_, CB_;
    std::mutex mu_;
    std::condition_variable pump_cv_, space_cv_, done_cv_;
    std::vector<Msg> slots_;
    std::vector<uint32_t> free_slots_, free_chunks_;
    std::set<uint64_t> open_;  // finished, not yet completed (by order of finish)
    uint64_t next_seq_ = 0, serial_ = 0;
    size_t live_ = 0, calls_ = 0;
    bool closing_ = false, stop_ = false, busy_ = false;
    uint64_t stat_[DS_STATS] = {};
    DsTick tick_[2];
    std::thread pump_;
};

}  // namespace nwv
