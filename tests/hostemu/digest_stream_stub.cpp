// The digest stream (narwhal_amd/csrc/digest_stream.h) over a stub device, with no GPU:
// tests/test_digest_stream_host.py drives the planner, the pump and the callbacks through this C
// interface.  The stub device keeps a "device" pool of its own, filled with a pattern: a tick's
// copies go from the planner's pinned pool into it, and its work records then run on it with
// blake2b.h's lane-local blake2b_compress exactly as k_blake2b_slice runs them (state per slot,
// DS_FIRST / DS_LAST, last_len, the digest by slot).  So a block that was never uploaded hashes
// the pattern, and the stub counts as violations: a block uploaded twice before it was consumed, a
// block consumed without an upload, a record outside the slice, the pool or the slots.
// Compiled with -DDSTREAM_STUB_MAIN the file is a stand-alone program (four submitting threads
// over a small pool), the form that test builds with -fsanitize=thread.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../narwhal_amd/csrc/blake2b.h"
#include "../../narwhal_amd/csrc/digest_stream.h"

namespace {

using namespace nwv;

struct StubDevice final : DsBackend {
    size_t S, P, M;
    std::vector<uint8_t> hpool, dpool, dig, up;
    std::vector<blake2b_state> st;
    std::atomic<uint64_t> violations{0}, copies{0}, copy_bytes{0}, busy_on{0}, busy_off{0}, max_rec_blocks{0},
        max_tick_recs{0}, dup_slots{0};
    StubDevice(size_t s, size_t p, size_t m)
        : S(s), P(p), M(m), hpool(p * s * 128, 0x5a), dpool(p * s * 128, 0xa5), dig(32 * m, 0), up(p * s, 0), st(m) {}
    uint8_t* host_pool() override { return hpool.data(); }
    const uint8_t* digests() override { return dig.data(); }
    void busy(bool on) override { (on ? busy_on : busy_off)++; }
    int wait(int) override { return 0; }
    int submit(int, const DsTick& t) override {
        for (const DsCopy& c : t.copies) {
            copies++;
            copy_bytes += c.len;
            if (c.off % 128 || c.len % 128 || c.off + c.len > dpool.size()) {
                violations++;
                continue;
            }
            for (uint64_t b = c.off / 128; b < (c.off + c.len) / 128; b++) {
                if (up[b]) violations++;  // uploaded twice
                up[b] = 1;
            }
            std::memcpy(dpool.data() + c.off, hpool.data() + c.off, c.len);
        }
        if (t.recs.size() > max_tick_recs) max_tick_recs = t.recs.size();
        std::vector<uint8_t> seen(M, 0);
        uint32_t prev = UINT32_MAX;
        for (const DsRecord& r : t.recs) {
            if (r.slot >= M || r.chunk >= P || r.first_block + (uint64_t)r.nblocks > S || r.nblocks == 0 ||
                r.last_len > 128 || r.nblocks > prev) {  // (longest first)
                violations++;
                continue;
            }
            prev = r.nblocks;
            if (seen[r.slot]++) dup_slots++;  // more than one record a message in a tick
            if (r.nblocks > max_rec_blocks) max_rec_blocks = r.nblocks;
            blake2b_state& s = st[r.slot];
            if (r.flags & DS_FIRST) blake2b_init256(s);
            for (uint32_t b = 0; b < r.nblocks; b++) {
                const size_t blk = (size_t)r.chunk * S + r.first_block + b;
                if (!up[blk]) violations++;  // consumed without an upload
                up[blk] = 0;
                u64p w[16];
                const uint8_t* p = dpool.data() + 128 * blk;
                for (int i = 0; i < 16; i++) {
                    std::memcpy(&w[i].lo, p + 8 * i, 4);
                    std::memcpy(&w[i].hi, p + 8 * i + 4, 4);
                }
                const bool last = (r.flags & DS_LAST) && b + 1 == r.nblocks;
                blake2b_compress(s, w, last ? r.last_len : 128u, last);
                std::memset(dpool.data() + 128 * blk, 0xa5, 128);  // a consumed block is gone
            }
            if (r.flags & DS_LAST) {
                uint32_t d[8];
                blake2b_digest256(s, d);
                std::memcpy(dig.data() + 32 * r.slot, d, 32);
            }
        }
        return 0;
    }
};

struct Result {
    std::atomic<int> fired{0};
    int32_t result = 0x7fffffff;
    uint8_t digest[32] = {};
    struct Harness* h = nullptr;
    uint64_t tag = 0;
    int mode = 0;  // 1: the callback calls flush and close; 2: it submits a chained message (tag + 1)
};

struct Harness {
    StubDevice dev;
    std::unique_ptr<DigestStream> ds;
    std::vector<std::unique_ptr<Result>> res;
    int reentrant[3] = {0, 0, 0};  // what flush, close and an oversized submit returned inside a callback
    std::vector<uint8_t> chained;  // what a mode-2 callback submits
    int chain_rc = 0x7fffffff;
    Harness(size_t s, size_t p, size_t m) : dev(s, p, m), ds(new DigestStream(dev, s, p, m)) {}
};

void on_done(void* user, int32_t result) {
    Result* r = static_cast<Result*>(user);
    r->result = result;
    r->fired++;
    Harness* h = r->h;
    if (r->mode == 1) {
        h->reentrant[0] = h->ds->flush();
        h->reentrant[1] = h->ds->close();
        // larger than the whole pool: it would have to wait for the pump, which is here
        std::vector<uint8_t> big(h->dev.hpool.size() + 1, 7);
        uint8_t sink[32];
        h->reentrant[2] = h->ds->submit(big.data(), big.size(), sink, nullptr, nullptr);
    } else if (r->mode == 2) {
        Result* nx = h->res[r->tag + 1].get();
        h->chain_rc = h->ds->submit(h->chained.data(), h->chained.size(), nx->digest, on_done, nx);
    }
}

}  // namespace

#ifndef DSTREAM_STUB_MAIN
extern "C" {

void* dsx_new(uint64_t slice, uint64_t chunks, uint64_t messages, uint64_t tags) {
    if (!DigestStream::config_ok(slice, chunks, messages)) return nullptr;
    Harness* h = new Harness(slice, chunks, messages);
    for (uint64_t i = 0; i < tags; i++) {
        h->res.emplace_back(new Result);
        h->res.back()->h = h;
        h->res.back()->tag = i;
    }
    return h;
}
void dsx_free(void* p) { delete static_cast<Harness*>(p); }
void dsx_set_mode(void* p, uint64_t tag, int mode) { static_cast<Harness*>(p)->res[tag]->mode = mode; }

int dsx_submit(void* p, const uint8_t* data, uint64_t len, uint64_t tag) {
    Harness* h = static_cast<Harness*>(p);
    Result* r = h->res[tag].get();
    return h->ds->submit(data, len, r->digest, on_done, r);
}
int dsx_submit_serialized(void* p, const uint8_t* buf, uint64_t len, uint64_t tag, int64_t* err) {
    Harness* h = static_cast<Harness*>(p);
    Result* r = h->res[tag].get();
    return h->ds->submit_serialized(buf, len, r->digest, err, on_done, r);
}
int dsx_begin(void* p, uint64_t tag, uint64_t* id) {
    Harness* h = static_cast<Harness*>(p);
    Result* r = h->res[tag].get();
    return h->ds->begin(r->digest, on_done, r, id);
}
int dsx_update(void* p, uint64_t id, const uint8_t* data, uint64_t len) {
    return static_cast<Harness*>(p)->ds->update(id, data, len);
}
int dsx_finish(void* p, uint64_t id) { return static_cast<Harness*>(p)->ds->finish(id); }
int dsx_flush(void* p) { return static_cast<Harness*>(p)->ds->flush(); }
int dsx_close(void* p) { return static_cast<Harness*>(p)->ds->close(); }
void dsx_stats(void* p, uint64_t out[8]) { static_cast<Harness*>(p)->ds->stats(out); }
// how often tag's callback fired; its result and digest
int dsx_result(void* p, uint64_t tag, int32_t* result, uint8_t digest[32]) {
    Result* r = static_cast<Harness*>(p)->res[tag].get();
    *result = r->result;
    std::memcpy(digest, r->digest, 32);
    return r->fired.load();
}
// out[0] violations, [1] copies issued, [2] bytes copied, [3] busy(true) calls, [4] busy(false) calls,
// [5] most blocks in one record, [6] most records in one tick, [7] ticks with two records of a slot
void dsx_device(void* p, uint64_t out[8]) {
    StubDevice& d = static_cast<Harness*>(p)->dev;
    out[0] = d.violations;
    out[1] = d.copies;
    out[2] = d.copy_bytes;
    out[3] = d.busy_on;
    out[4] = d.busy_off;
    out[5] = d.max_rec_blocks;
    out[6] = d.max_tick_recs;
    out[7] = d.dup_slots;
}
int dsx_set_chained(void* p, const uint8_t* data, uint64_t len) {
    static_cast<Harness*>(p)->chained.assign(data, data + len);
    return 0;
}
int dsx_chain_rc(void* p) { return static_cast<Harness*>(p)->chain_rc; }
void dsx_reentrant(void* p, int out[3]) { std::memcpy(out, static_cast<Harness*>(p)->reentrant, sizeof(int) * 3); }
// the bincode walk alone
int64_t dsx_walk(const uint8_t* buf, uint64_t len, uint64_t* payload) {
    std::vector<DsSeg> segs;
    const int64_t e = ds_walk_batch(buf, len, segs);
    *payload = 0;
    for (const DsSeg& s : segs) *payload += s.len;
    return e;
}

}  // extern "C"
#else
// one-shot BLAKE2b-256 with the same compression (the program's own reference)
static void oneshot(const uint8_t* msg, size_t len, uint8_t out[32]) {
    blake2b_state s;
    blake2b_init256(s);
    const size_t nb = len == 0 ? 1 : (len + 127) / 128;
    for (size_t b = 0; b < nb; b++) {
        uint8_t blk[128] = {};
        const size_t n = std::min<size_t>(128, len - 128 * b);
        std::memcpy(blk, msg + 128 * b, n);
        u64p w[16];
        for (int i = 0; i < 16; i++) {
            std::memcpy(&w[i].lo, blk + 8 * i, 4);
            std::memcpy(&w[i].hi, blk + 8 * i + 4, 4);
        }
        const bool last = b + 1 == nb;
        blake2b_compress(s, w, last ? (uint32_t)n : 128u, last);
    }
    uint32_t d[8];
    blake2b_digest256(s, d);
    std::memcpy(out, d, 32);
}

int main() {
    const int threads = 4, per = 200;
    Harness h(4, 16, 8);
    for (int i = 0; i < threads * per; i++) {
        h.res.emplace_back(new Result);
        h.res.back()->h = &h;
    }
    std::vector<std::vector<uint8_t>> msgs(threads * per);
    for (int i = 0; i < threads * per; i++) {
        msgs[i].resize((size_t)((i * 2654435761u) % 3000));
        for (size_t k = 0; k < msgs[i].size(); k++) msgs[i][k] = (uint8_t)(i * 31 + k * 7);
    }
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int k = 0; k < threads; k++)
        th.emplace_back([&, k] {
            for (int j = 0; j < per; j++) {
                const int i = k * per + j;
                Result* r = h.res[i].get();
                if (j % 3 == 0) {  // piecewise
                    uint64_t id = 0;
                    if (h.ds->begin(r->digest, on_done, r, &id)) bad++;
                    for (size_t o = 0; o < msgs[i].size(); o += 129)
                        if (h.ds->update(id, msgs[i].data() + o, std::min<size_t>(129, msgs[i].size() - o))) bad++;
                    if (h.ds->finish(id)) bad++;
                } else if (h.ds->submit(msgs[i].data(), msgs[i].size(), r->digest, on_done, r)) {
                    bad++;
                }
            }
            if (h.ds->flush()) bad++;
        });
    for (auto& x : th) x.join();
    bool ok = bad == 0 && h.ds->close() == 0 && h.dev.violations == 0 && h.dev.dup_slots == 0;
    uint64_t st[8];
    h.ds->stats(st);
    for (int i = 0; i < threads * per; i++) {
        uint8_t want[32];
        oneshot(msgs[i].data(), msgs[i].size(), want);
        ok = ok && h.res[i]->fired == 1 && h.res[i]->result == 0 && std::memcmp(want, h.res[i]->digest, 32) == 0;
    }
    ok = ok && st[DS_STAT_MESSAGES] == (uint64_t)threads * per && st[DS_STAT_CHUNKS] == 0 &&
         st[DS_STAT_CHUNKS_PEAK] <= 16;
    std::printf("digest stream hammer: %llu messages, %s\n", (unsigned long long)st[DS_STAT_MESSAGES],
                ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
