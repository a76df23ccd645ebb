// bls_wave_vectors.hip -- the device's wave interpreter (bls_wave.h), fp_inv_wave and the F == 1
// verdicts on slot images from a file, one 64-lane workgroup per case, all cases in one launch
// (tests/test_gpu_bls_wave_vectors.py; tests/bls_wave_vectors.py builds the images and what must
// come out).
//   bls_wave_vectors IN OUT
// IN (little-endian u32 words): magic, cases, payload words in, payload words out; then 8 words per
// case: mode, program offset, stages, first stage's lanes, reps, k, slots, 0; then the payloads in
// case order.  OUT: the cases' results in case order.
//   RUN1   in: `slots` slots (14 words each) from slot 0 on (the rest of the wave's NSLOTS start as
//          zero); Wave::run(program, reps), the real wave_run; out: the same slots
//   RUNK   in: k banks of NSLOTS_PC slots behind one shared P << k table (the packed pairing
//          kernel's layout); every lane of a stage calls lane_value<NWV_BLS_PAIR_TERMS>(bank, table,
//          ..) for each bank; out: the banks.  (The packed kernel's own lane-to-item loop is inline
//          in pair_flat and is not repeated here.)
//   INV    in: one value; out: fp_inv_wave's result of each of the 64 lanes
//   ISONE  in: the 12 F slots of each of k banks; out: per lane WaveK::f_is_one_mask() |
//          (bit j: Wave::f_is_one() on bank j) << 8
// The whole input is validated before anything is launched: every program's records must lie
// inside T_DATA and address only slots the case has, and the counts are capped.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../narwhal_amd/csrc/bls_wave.h"

using namespace bls;
using namespace bls::wave;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

enum : uint32_t { M_RUN1 = 0, M_RUNK = 1, M_INV = 2, M_ISONE = 3 };
constexpr uint32_t MAGIC = 0x31565742u;  // "BWV1"
constexpr uint32_t MAX_CASES = 8192, MAX_REPS = 8, MAX_K = 4, MAX_WORDS = 1u << 26;
constexpr uint32_t BANKW = (uint32_t)(SW * NSLOTS_PC);
constexpr uint32_t SLOT_WORDS = SW * NSLOTS > MAX_K * BANKW ? SW * NSLOTS : MAX_K * BANKW;
constexpr uint32_t LDS_WORDS = KP_WORDS + SLOT_WORDS;
constexpr size_t TDATA_LEN = sizeof(T_DATA) / sizeof(T_DATA[0]);

struct Case {
    uint32_t mode, off, n, nl0, reps, k, slots, in_off, out_off;
};

__global__ __launch_bounds__(64) void k_bls_wave_vectors(const Case* cases, const uint32_t* in, uint32_t* out) {
    extern __shared__ uint32_t lds[];
    const Case c = cases[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint32_t* src = in + c.in_off;
    uint32_t* dst = out + c.out_off;
    for (int t = lane; t < KP_WORDS; t += 64) lds[t] = (&T_KP[0][0])[t];
    uint32_t* wm = lds + KP_WORDS;
    if (c.mode == M_RUN1) {
        const int nw = SW * (int)c.slots;
        for (int t = lane; t < SW * NSLOTS; t += 64) wm[t] = t < nw ? src[t] : 0u;
        wsync();
        const Wave w{wm, lane};
        w.run(Prog{c.off, (uint16_t)c.n, (uint16_t)c.nl0}, (int)c.reps);
        for (int t = lane; t < nw; t += 64) dst[t] = wm[t];
    } else if (c.mode == M_RUNK) {
        const int nw = (int)(c.k * BANKW);
        for (int t = lane; t < nw; t += 64) wm[t] = src[t];
        wsync();
        const wword* kpt = (const wword*)lds;
#pragma unroll 1
        for (uint32_t rep = 0; rep < c.reps; rep++) {
            const uint16_t* base = T_DATA + c.off;
            int nl = (int)c.nl0;
#pragma unroll 1
            for (uint32_t s = 0; s < c.n; s++) {
                const Rec cur = load_rec(base + (uint32_t)min(lane, nl - 1) * REC);
                Hdr h = rec_hdr(cur);
                h.nap = __builtin_amdgcn_readfirstlane(h.nap);
                h.nan = __builtin_amdgcn_readfirstlane(h.nan);
                h.nbp = __builtin_amdgcn_readfirstlane(h.nbp);
                h.nbn = __builtin_amdgcn_readfirstlane(h.nbn);
                if (lane < nl) {
                    const uint32_t d = rec_u16(cur, 0);
#pragma unroll 1
                    for (uint32_t j = 0; j < c.k; j++) {
                        wword* bank = (wword*)(wm + j * BANKW);
                        const fp v = lane_value<NWV_BLS_PAIR_TERMS>(bank, kpt, h, cur);
#pragma unroll
                        for (int i = 0; i < NL; i++) bank[SW * d + i] = v.l[i];
                    }
                }
                wsync();
                base += (uint32_t)nl * REC;
                nl = __builtin_amdgcn_readfirstlane(h.nl_next);
            }
        }
        for (int t = lane; t < nw; t += 64) dst[t] = wm[t];
    } else if (c.mode == M_INV) {
        fp x;
        for (int j = 0; j < NL; j++) x.l[j] = src[j];
        const fp r = fp_inv_wave(x);
        for (int j = 0; j < NL; j++) dst[NL * lane + j] = r.l[j];
    } else {
        for (uint32_t j = 0; j < c.k; j++)
            for (int t = lane; t < 12 * SW; t += 64) wm[j * BANKW + SW * REG_F + t] = src[j * 12 * SW + t];
        wsync();
        const WaveK wk{wm, BANKW, (int)c.k, lane};
        const uint32_t mask = wk.f_is_one_mask();
        uint32_t bits = 0;
        for (uint32_t j = 0; j < c.k; j++) {
            const Wave w{wm + j * BANKW, lane};
            if (w.f_is_one()) bits |= 1u << j;
        }
        dst[lane] = mask | (bits << 8);
    }
}

// the program's records lie inside `data` (a copy of T_DATA) and address slots below `nslots` only
static bool prog_ok(const uint16_t* data, uint32_t off, uint32_t n, uint32_t nl0, uint32_t nslots) {
    if (n < 1 || n > 64 || off % 8 || off >= TDATA_LEN) return false;
    size_t at = off;
    uint32_t nl = nl0;
    for (uint32_t s = 0; s < n; s++) {
        // (the table ends in two spare records, which a lane's 16-byte loads may touch)
        if (nl < 1 || nl > 64 || at + (size_t)nl * REC + 2 * REC > TDATA_LEN) return false;
        uint32_t nl_next = 0;
        for (uint32_t l = 0; l < nl; l++) {
            const uint16_t* r = data + at + (size_t)l * REC;
            if (r[REC - 4] != nl || r[0] >= nslots || r[2] > 16 || r[3] > 16) return false;
            for (int t = 4; t < 4 + 4 * TMAX; t++)
                if ((r[t] & 0xfffu) >= nslots) return false;
            if (l && r[REC - 1] != nl_next) return false;
            nl_next = r[REC - 1];
        }
        at += (size_t)nl * REC;
        nl = nl_next;
    }
    return true;
}

static int bad(const char* what, uint32_t i) {
    fprintf(stderr, "bls_wave_vectors: case %u: %s\n", i, what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: bls_wave_vectors IN OUT\n");
        return 1;
    }
    FILE* fi = fopen(argv[1], "rb");
    uint32_t hdr[4];
    if (!fi || fread(hdr, 4, 4, fi) != 4 || hdr[0] != MAGIC || hdr[1] == 0 || hdr[1] > MAX_CASES ||
        hdr[2] > MAX_WORDS || hdr[3] == 0 || hdr[3] > MAX_WORDS) {
        fprintf(stderr, "bls_wave_vectors: cannot read %s or its header is out of range\n", argv[1]);
        return 1;
    }
    const uint32_t nc = hdr[1];
    std::vector<uint32_t> tab(8 * (size_t)nc), payload(hdr[2]);
    uint32_t extra;
    if (fread(tab.data(), 4, tab.size(), fi) != tab.size() ||
        fread(payload.data(), 4, payload.size(), fi) != payload.size() || fread(&extra, 1, 1, fi) != 0) {
        fprintf(stderr, "bls_wave_vectors: the length of %s does not match its header\n", argv[1]);
        return 1;
    }
    fclose(fi);
    // counts, sizes and offsets first (no GPU call yet)
    std::vector<Case> cases(nc);
    uint64_t nin = 0, nout = 0;
    for (uint32_t i = 0; i < nc; i++) {
        const uint32_t* t = &tab[8 * (size_t)i];
        Case& c = cases[i];
        c = Case{t[0], t[1], t[2], t[3], t[4], t[5], t[6], (uint32_t)nin, (uint32_t)nout};
        uint64_t wi, wo;
        if (c.mode == M_RUN1) {
            if (c.slots < 1 || c.slots > (uint32_t)NSLOTS || c.k != 1) return bad("slots or k", i);
            wi = wo = (uint64_t)SW * c.slots;
        } else if (c.mode == M_RUNK) {
            if (c.k < 1 || c.k > MAX_K || c.slots != (uint32_t)NSLOTS_PC) return bad("k or slots", i);
            wi = wo = (uint64_t)c.k * BANKW;
        } else if (c.mode == M_INV) {
            wi = NL;
            wo = 64 * NL;
        } else if (c.mode == M_ISONE) {
            if (c.k < 1 || c.k > MAX_K) return bad("k", i);
            wi = (uint64_t)c.k * 12 * SW;
            wo = 64;
        } else {
            return bad("mode", i);
        }
        if (c.mode <= M_RUNK && (c.reps < 1 || c.reps > MAX_REPS || c.n < 1 || c.n > 64 || c.nl0 < 1 || c.nl0 > 64))
            return bad("reps, stages or lanes", i);
        nin += wi;
        nout += wo;
        if (nin > hdr[2] || nout > hdr[3]) return bad("payload beyond the header's count", i);
    }
    if (nin != hdr[2] || nout != hdr[3]) {
        fprintf(stderr, "bls_wave_vectors: the cases take %llu words in and %llu out, the header says %u and %u\n",
                (unsigned long long)nin, (unsigned long long)nout, hdr[2], hdr[3]);
        return 1;
    }
    // every program against the device's own record table
    std::vector<uint16_t> data(TDATA_LEN);
    CHECK(hipMemcpyFromSymbol(data.data(), HIP_SYMBOL(T_DATA), sizeof(T_DATA)));
    for (uint32_t i = 0; i < nc; i++) {
        const Case& c = cases[i];
        if (c.mode <= M_RUNK && !prog_ok(data.data(), c.off, c.n, c.nl0, c.slots))
            return bad("the program leaves T_DATA or the case's slots", i);
    }
    Case* dc;
    uint32_t *din, *dout;
    CHECK(hipMalloc(&dc, sizeof(Case) * (size_t)nc));
    CHECK(hipMalloc(&din, 4 * (payload.size() + 1)));
    CHECK(hipMalloc(&dout, 4 * (size_t)hdr[3]));
    CHECK(hipMemcpy(dc, cases.data(), sizeof(Case) * (size_t)nc, hipMemcpyHostToDevice));
    if (!payload.empty()) CHECK(hipMemcpy(din, payload.data(), 4 * payload.size(), hipMemcpyHostToDevice));
    CHECK(hipMemset(dout, 0, 4 * (size_t)hdr[3]));
    hipLaunchKernelGGL(k_bls_wave_vectors, dim3(nc), dim3(64), 4 * LDS_WORDS, 0, dc, din, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> res(hdr[3]);
    CHECK(hipMemcpy(res.data(), dout, 4 * res.size(), hipMemcpyDeviceToHost));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo || fwrite(res.data(), 4, res.size(), fo) != res.size() || fclose(fo) != 0) {
        fprintf(stderr, "bls_wave_vectors: cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}
