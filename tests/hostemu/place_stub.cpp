// The placement policy of a multi-device context (narwhal_amd/csrc/place.h) behind a C interface,
// with no HIP: tests/test_place_host.py drives the load table, the tickets and the rotation of
// split calls through it.  Compiled with -DPLACE_STUB_MAIN the file is a stand-alone program that
// runs the threaded pick-and-release loop and checks the table afterwards (the form that test
// builds with -fsanitize=thread).
#include <cstdint>
#include <cstdio>
#include <thread>
#include <utility>
#include <vector>

#include "../../narwhal_amd/csrc/place.h"

namespace {

// `threads` host threads, each `iters` times: place a single-range call of 1 + (i mod 7) items and
// release it.  Returns the picks made; per_dev[d] (when given) counts the picks that device d got.
uint64_t hammer(nwv::PlaceTable& t, int threads, int iters, uint64_t* per_dev) {
    std::vector<std::vector<uint64_t>> got(threads, std::vector<uint64_t>(t.size(), 0));
    std::vector<std::thread> th;
    for (int k = 0; k < threads; k++)
        th.emplace_back([&, k]() {
            for (int i = 0; i < iters; i++) {
                nwv::Ticket tk(t, (uint64_t)(1 + i % 7));
                got[k][tk.dev()]++;
            }
        });
    for (auto& x : th) x.join();
    uint64_t total = 0;
    for (int k = 0; k < threads; k++)
        for (size_t d = 0; d < t.size(); d++) {
            total += got[k][d];
            if (per_dev) per_dev[d] += got[k][d];
        }
    return total;
}

// a call that takes its ticket and then fails: the early return is the error path
int failing_call(nwv::PlaceTable& t, uint64_t items, int fail, int* dev) {
    nwv::Ticket tk(t, items);
    *dev = (int)tk.dev();
    if (fail) return fail;
    return 0;
}

}  // namespace

#ifndef PLACE_STUB_MAIN
extern "C" {

void* pl_new(uint64_t ndev, int first) {
    return new nwv::PlaceTable((size_t)ndev, first ? nwv::PLACE_FIRST : nwv::PLACE_LOAD);
}
void pl_free(void* t) { delete static_cast<nwv::PlaceTable*>(t); }
int pl_env_first(void) { return nwv::place_mode_from_env() == nwv::PLACE_FIRST; }

// a single-range call's ticket (placed by the table) / a range's ticket on a named device
void* pl_pick(void* t, uint64_t items, int engine) {
    return new nwv::Ticket(*static_cast<nwv::PlaceTable*>(t), items, engine);
}
void* pl_acquire(void* t, uint64_t dev, uint64_t items, int engine) {
    return new nwv::Ticket(*static_cast<nwv::PlaceTable*>(t), (size_t)dev, items, engine);
}
int pl_ticket_dev(void* tk) { return (int)static_cast<nwv::Ticket*>(tk)->dev(); }
void pl_release(void* tk) { delete static_cast<nwv::Ticket*>(tk); }

// a call of k ranges of `per` items each, as for_shards places it: devs[j] = range j's device;
// the tickets are released before the function returns (the call has returned)
int pl_call_ranges(void* t, int k, uint64_t per, int engine, int32_t* devs) {
    std::vector<std::pair<size_t, size_t>> r;
    for (int j = 0; j < k; j++) r.push_back({(size_t)(j * per), (size_t)((j + 1) * per)});
    const auto tickets = nwv::place_ranges(*static_cast<nwv::PlaceTable*>(t), r, engine);
    for (size_t j = 0; j < tickets.size(); j++) devs[j] = (int32_t)tickets[j].dev();
    return (int)tickets.size();
}
int pl_failing_call(void* t, uint64_t items, int fail, int* dev) {
    return failing_call(*static_cast<nwv::PlaceTable*>(t), items, fail, dev);
}

// out[0] outstanding ranges, [1] outstanding items, [2] peak, [3] ranges and [4] items placed by
// engine 0, [5] and [6] by engine 1
void pl_get(void* t, uint64_t dev, uint64_t out[7]) {
    const nwv::PlaceEntry e = static_cast<nwv::PlaceTable*>(t)->get((size_t)dev);
    out[0] = e.out_ranges;
    out[1] = e.out_items;
    out[2] = e.peak;
    out[3] = e.ranges[0];
    out[4] = e.items[0];
    out[5] = e.ranges[1];
    out[6] = e.items[1];
}

uint64_t pl_hammer(void* t, int threads, int iters, uint64_t* per_dev) {
    return hammer(*static_cast<nwv::PlaceTable*>(t), threads, iters, per_dev);
}

}  // extern "C"
#else
int main() {
    const int threads = 8, iters = 10000;
    nwv::PlaceTable t(3);
    std::vector<uint64_t> per(t.size(), 0);
    const uint64_t picks = hammer(t, threads, iters, per.data());
    uint64_t ranges = 0;
    bool ok = picks == (uint64_t)threads * iters;
    for (size_t d = 0; d < t.size(); d++) {
        const nwv::PlaceEntry e = t.get(d);
        ranges += e.ranges[0];
        ok = ok && e.ranges[0] == per[d] && e.out_ranges == 0 && e.out_items == 0 && e.peak <= (uint64_t)threads;
    }
    ok = ok && ranges == picks;
    int dev = -1;
    ok = ok && failing_call(t, 5, 7, &dev) == 7 && dev == 0 && t.get(0).out_ranges == 0;
    std::printf("place hammer: %llu picks, %s\n", (unsigned long long)picks, ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
#endif
