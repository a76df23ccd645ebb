// blake2b_kernels.hip -- K6: BLAKE2b-256 digests on gfx950.
//
//   k_blake2b_many     one message per lane (header / vote / certificate digests, many
//                      independent batches): fastcrypto::blake2b_256 semantics
//   k_batch_compact    one workgroup per bincode WorkerMessage::Batch buffer: walks the
//                      [u32 variant][u64 count][(u64 len, bytes)]* layout of
//                      types/src/worker.rs:44-80 and packs the transaction bytes (the
//                      Batch::digest stream, types/src/primary.rs:65-73) contiguously; the
//                      packed streams are then hashed by k_blake2b_many.
// Message arenas are padded by >= 16 bytes (aligned over-reads are safe).
#include "blake2b.h"

using namespace nwv;

// out2 (optional): a second copy of the digests (coherent pinned host memory: no copy back)
extern "C" __global__ void __launch_bounds__(256) k_blake2b_many(
    uint64_t n, const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
    const uint64_t* __restrict__ len, uint32_t* __restrict__ out, uint32_t* __restrict__ out2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = base + off[i];
    const uint64_t L = len[i];
    blake2b_state s;
    blake2b_init256(s);
    const uint64_t nblocks = L == 0 ? 1 : (L + 127) / 128;
#pragma unroll 1
    for (uint64_t b = 0; b < nblocks; b++) {
        u64p m[16];
        const uint64_t pos0 = 128 * b;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            m[t].lo = msg_word_trim(p, pos0 + 8 * t, L);
            m[t].hi = msg_word_trim(p, pos0 + 8 * t + 4, L);
        }
        const bool last = b + 1 == nblocks;
        blake2b_compress(s, m, last ? (uint32_t)(L - pos0) : 128u, last);
    }
    uint32_t d[8];
    blake2b_digest256(s, d);
    uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
    if (out2) {
        uint4* o2 = reinterpret_cast<uint4*>(out2 + 8 * i);
        o2[0] = make_uint4(d[0], d[1], d[2], d[3]);
        o2[1] = make_uint4(d[4], d[5], d[6], d[7]);
    }
}

// ---- long messages: 4 lanes per message --------------------------------------------------
// BLAKE2b is sequential over blocks, so a worker batch (types/src/primary.rs:65-73, ~500 KB =
// 3,909 compressions) is latency-bound on one lane.  Here the 4 lanes of a quad hold the 4
// columns of the 4x4 state (lane q: v[q], v[q+4], v[q+8], v[q+12]) and run the column step's
// and the diagonal step's G functions in parallel; between the two steps rows 1-3 rotate
// across the quad with DPP quad_perm moves.  The 128-byte block is staged in LDS (each lane
// loads 32 bytes) and every G reads its two sigma-selected words from there.
namespace {
// quad_perm controls: lane q reads lane (q+1)%4, (q+2)%4, (q+3)%4
constexpr int QP_NEXT1 = 0x39, QP_NEXT2 = 0x4E, QP_NEXT3 = 0x93;
// update_dpp with bound_ctrl (every lane of a quad_perm reads a live lane, so the zero fill never
// applies): in that form LLVM folds the move into a VOP2 consumer as a DPP source operand
// (v_xor_b32_dpp for d ^ a), 44 fewer instructions per compression
template <int CTRL>
__device__ __forceinline__ uint64_t quad_rot(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, true);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// rotation as two independent v_alignbit_b32 on the halves (one dependent level; the shift/or
// form the compiler picks for (x >> n) | (x << (64 - n)) is two)
__device__ __forceinline__ uint64_t rotr64(uint64_t x, int n) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (n == 32) return ((uint64_t)lo << 32) | hi;
    const u64p r = rotr(u64p{lo, hi}, n);
    return ((uint64_t)r.hi << 32) | r.lo;
}
// G on native 64-bit words: the adds become single v_lshl_add_u64 (gfx950).  The message word is
// added to a before b is (a + m does not wait for b, the previous G's last result), so each half
// of G has one dependent add less on the chain that bounds a long message's latency.
// opaque to reassociation: LLVM would otherwise rewrite (a + m) + b as (m + b) + a
__device__ __forceinline__ uint64_t pinned_sum(uint64_t a, uint64_t m) {
    uint64_t t = a + m;
    __asm__("" : "+v"(t));
    return t;
}
__device__ __forceinline__ void b2_g(uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d, uint64_t x, uint64_t y) {
    a = b + pinned_sum(a, x);
    d = rotr64(d ^ a, 32);
    c = c + d;
    b = rotr64(b ^ c, 24);
    a = b + pinned_sum(a, y);
    d = rotr64(d ^ a, 16);
    c = c + d;
    b = rotr64(b ^ c, 63);
}
// nibble q of the packed sigma entries for lane q
constexpr uint32_t sigma_pack(int r, int first) {
    uint32_t v = 0;
    for (int q = 0; q < 4; q++) v |= (uint32_t)BLAKE2B_SIGMA[r][first + 2 * q] << (4 * q);
    return v;
}
__device__ __forceinline__ uint64_t iv64(int k) {
    return (uint64_t)BLAKE2B_IV32[2 * k] | ((uint64_t)BLAKE2B_IV32[2 * k + 1] << 32);
}
}  // namespace

// The quad form on one wave: messages 16 * group .. 16 * group + 15 of the call, blk = the wave's
// 16 staged blocks in LDS.  BLOCK_SYNC: the wave is the whole workgroup (k_blake2b_quad) and the
// staging is ordered by the workgroup barrier; otherwise (the digest workgroups of the fused typed
// kernels, tiny_kernels.hip / comb_kernels.hip, where each wave runs groups of its own and waves
// loop different numbers of times) by the wave's own in-order LDS pipe, with no barrier at all.
template <bool BLOCK_SYNC>
__device__ __forceinline__ void b2_quad_sync() {
    if (BLOCK_SYNC) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
template <bool BLOCK_SYNC>
__device__ __forceinline__ void b2_quad_group(uint64_t (*blk)[16], int lane, uint64_t group, uint64_t n,
                                              const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                              const uint64_t* __restrict__ len, uint32_t* __restrict__ out,
                                              uint32_t* __restrict__ out2) {
    const int q = lane & 3, slot = lane >> 2;
    const uint64_t i = group * 16 + slot;
    const bool active = i < n;
    const uint8_t* p = active ? base + off[i] : base;
    const uint64_t L = active ? len[i] : 0;
    const uint64_t nb = active ? (L == 0 ? 1 : (L + 127) / 128) : 0;
    uint64_t nmax = nb;  // blocks of the longest message of the wave
    for (int o = 4; o < 64; o <<= 1) {
        const uint64_t t = __shfl_xor(nmax, o);
        nmax = t > nmax ? t : nmax;
    }
    const uint64_t iv0 = iv64(q), iv1 = iv64(q + 4);
    uint64_t h0 = iv0, h1 = iv1;
    if (q == 0) h0 ^= 0x01010000u ^ 32u;
    const int sh = 4 * q;
    // the next block's 32 bytes for this lane are fetched one block ahead (9 aligned dwords
    // cover an unaligned 32-byte window), so the global-load latency overlaps a compression
    uint32_t raw[9];
    auto fetch = [&](uint64_t blk_idx) {
        const uintptr_t a = (uintptr_t)(p + 128 * blk_idx + 32 * q);
        const uint32_t* wp = (const uint32_t*)(a & ~(uintptr_t)3);
#pragma unroll
        for (int t = 0; t < 9; t++) raw[t] = wp[t];
    };
    if (nb > 0) fetch(0);
#pragma unroll 1
    for (uint64_t b = 0; b < nmax; b++) {
        const bool live = b < nb;
        const uint64_t pos = 128 * b + 32 * q;
        const uint32_t ash = (uint32_t)(((uintptr_t)(p + pos)) & 3) * 8;
        uint32_t w[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const uint64_t two = ((uint64_t)raw[t + 1] << 32) | raw[t];
            uint32_t v = (uint32_t)(two >> ash);
            const uint64_t bp = pos + 4 * t;  // trim to the message length (zero past the end)
            if (!live || bp >= L) v = 0u;
            else if (bp + 4 > L) v &= 0xffffffffu >> (8 * (uint32_t)(bp + 4 - L));
            w[t] = v;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) blk[slot][4 * q + t] = (uint64_t)w[2 * t] | ((uint64_t)w[2 * t + 1] << 32);
        if (b + 1 < nb) fetch(b + 1);
        b2_quad_sync<BLOCK_SYNC>();
        // every sigma-selected word this lane needs for the 12 rounds, before the chain starts
        const uint64_t* m = blk[slot];
        uint64_t mw[12][4];
#pragma unroll
        for (int r = 0; r < 12; r++) {
            mw[r][0] = m[(sigma_pack(r, 0) >> sh) & 15];
            mw[r][1] = m[(sigma_pack(r, 1) >> sh) & 15];
            mw[r][2] = m[(sigma_pack(r, 8) >> sh) & 15];
            mw[r][3] = m[(sigma_pack(r, 9) >> sh) & 15];
        }
        const bool last = b + 1 == nb;
        const uint64_t tb = last ? L : 128 * (b + 1);  // bytes compressed so far
        uint64_t va = h0, vb = h1, vc = iv0, vd = iv1;
        if (q == 0) vd ^= tb;
        if (q == 2 && last) vd = ~vd;
#pragma unroll
        for (int r = 0; r < 12; r++) {
            b2_g(va, vb, vc, vd, mw[r][0], mw[r][1]);
            vb = quad_rot<QP_NEXT1>(vb);
            vc = quad_rot<QP_NEXT2>(vc);
            vd = quad_rot<QP_NEXT3>(vd);
            b2_g(va, vb, vc, vd, mw[r][2], mw[r][3]);
            vb = quad_rot<QP_NEXT3>(vb);
            vc = quad_rot<QP_NEXT2>(vc);
            vd = quad_rot<QP_NEXT1>(vd);
        }
        if (live) {
            h0 ^= va ^ vc;
            h1 ^= vb ^ vd;
        }
        b2_quad_sync<BLOCK_SYNC>();
    }
    if (active) {
        out[8 * i + 2 * q] = (uint32_t)h0;
        out[8 * i + 2 * q + 1] = (uint32_t)(h0 >> 32);
        if (out2) {
            out2[8 * i + 2 * q] = (uint32_t)h0;
            out2[8 * i + 2 * q + 1] = (uint32_t)(h0 >> 32);
        }
    }
}

extern "C" __global__ void __launch_bounds__(64) k_blake2b_quad(
    uint64_t n, const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
    const uint64_t* __restrict__ len, uint32_t* __restrict__ out, uint32_t* __restrict__ out2) {
    __shared__ uint64_t blk[16][16];
    b2_quad_group<true>(blk, (int)threadIdx.x, (uint64_t)blockIdx.x, n, base, off, len, out, out2);
}

// The "side" digests of a fused typed call (k_ed_tiny_fused / k_ed_comb_fused): the workgroups
// past the signature workgroups hash the call's long preimages with the quad form, B2_SIDE_WAVES
// waves a workgroup and 16 messages a wave; later waves of the workgroup leave at once.  Nothing
// here touches the verdict words or waits for anybody.
static constexpr int B2_SIDE_WAVES = 2;
struct B2SideArgs {
    uint64_t n;            // side preimages (0: the launch has no digest workgroups)
    const uint8_t* base;
    const uint64_t* off;
    const uint64_t* len;
    uint32_t* out;         // device digests [n][8]
    uint32_t* out2;        // coherent pinned host memory [n][8], or null
};
__device__ __forceinline__ void b2_side_block(const B2SideArgs& s, uint32_t block) {
    __shared__ uint64_t sblk[B2_SIDE_WAVES][16][16];
    const int wv = (int)(threadIdx.x >> 6);
    if (wv >= B2_SIDE_WAVES) return;
    const uint64_t group = (uint64_t)block * B2_SIDE_WAVES + (uint64_t)wv;
    if (group * 16 >= s.n) return;  // (wave-uniform)
    b2_quad_group<false>(sblk[wv], (int)(threadIdx.x & 63), group, s.n, s.base, s.off, s.len, s.out, s.out2);
}

namespace {
__device__ __forceinline__ uint64_t ld_u64_unaligned(const uint8_t* p) {
    return (uint64_t)ld_u32_unaligned(p) | ((uint64_t)ld_u32_unaligned(p + 4) << 32);
}
}  // namespace

// One workgroup per serialized batch i (buffer base + off[i], len[i] bytes).  Lane 0 walks
// the length prefixes (a dependent chain by construction of the format) and records the
// segments in LDS in chunks; all lanes then copy each chunk's transaction bytes into
// packed + off[i] (payload <= len[i] - 12).  payload_len[i] = packed length, or err[i] =
// offset of the u64 field that could not be read (DigestError::InvalidArgumentError).
static constexpr int SEG_CHUNK = 1024;
extern "C" __global__ void __launch_bounds__(256) k_batch_compact(
    uint64_t n, const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
    const uint64_t* __restrict__ len, uint8_t* __restrict__ packed,
    uint64_t* __restrict__ payload_len, int64_t* __restrict__ err) {
    const uint64_t i = blockIdx.x;
    if (i >= n) return;
    __shared__ uint64_t seg_src[SEG_CHUNK];
    __shared__ uint64_t seg_dst[SEG_CHUNK];
    __shared__ uint64_t seg_len[SEG_CHUNK];
    __shared__ int nseg;
    __shared__ int done;
    __shared__ int64_t err_off;
    __shared__ uint64_t walk_pos, walk_left, walk_dst;
    const uint8_t* buf = base + off[i];
    uint8_t* dst = packed + off[i];
    const uint64_t L = len[i];
    if (threadIdx.x == 0) {
        err_off = -1;
        done = 0;
        walk_dst = 0;
        if (L < 12) {
            err_off = 4;
            done = 1;
        } else {
            walk_left = ld_u64_unaligned(buf + 4);
            walk_pos = 12;
        }
    }
    __syncthreads();
    if (done) {
        if (threadIdx.x == 0) { err[i] = err_off; payload_len[i] = 0; }
        return;
    }
    for (;;) {
        if (threadIdx.x == 0) {
            int k = 0;
            uint64_t pos = walk_pos, left = walk_left, d = walk_dst;
            while (left > 0 && k < SEG_CHUNK) {
                if (pos + 8 > L) { err_off = (int64_t)pos; break; }
                const uint64_t tl = ld_u64_unaligned(buf + pos);
                if (tl > L - pos - 8) { err_off = (int64_t)pos; break; }
                seg_src[k] = pos + 8;
                seg_dst[k] = d;
                seg_len[k] = tl;
                d += tl;
                pos += 8 + tl;
                left--;
                k++;
            }
            nseg = k;
            walk_pos = pos;
            walk_left = left;
            walk_dst = d;
            done = (left == 0 || err_off >= 0) ? 1 : 0;
        }
        __syncthreads();
        const bool finished = done != 0;  // read between the two barriers: stable
        // copy this chunk's segments: lanes stride over the bytes of each segment
        for (int s = 0; s < nseg; s++) {
            const uint64_t sl = seg_len[s], ss = seg_src[s], sd = seg_dst[s];
            for (uint64_t b = threadIdx.x; b < sl; b += blockDim.x) dst[sd + b] = buf[ss + b];
        }
        __syncthreads();
        if (finished) break;
    }
    if (threadIdx.x == 0) {
        err[i] = err_off;
        payload_len[i] = err_off >= 0 ? 0 : walk_dst;
    }
}

// ---- resumable slices of long messages (the digest stream, digest_stream.h) ----------------------
// The quad form of k_blake2b_quad, one work record (nwv::DsRecord, 8 dwords) a quad: run `nblocks`
// compressions from block `first_block` of pool chunk `chunk` on the chaining value of message slot
// `slot`.  state holds 16 words a slot (h[8], the byte counter t, 7 unused); a record flagged
// DS_FIRST starts from the IV and parameter block instead of loading, every record stores the state
// back, and one flagged DS_LAST compresses its final block with t += last_len (0..128) and the
// finalisation flag, then stores the digest at 32 * slot of out and out2 (coherent pinned host
// memory).  Chunks are 128-byte aligned and zero-padded by the host, so lane q loads its 32 bytes
// of a block with two aligned 16-byte loads, one block ahead, and nothing is trimmed.
// Fail closed: a slot >= n_slots is dropped, chunk is clamped to the pool, first_block and
// nblocks to the slice, last_len to 128: no record loops longer than slice_blocks compressions or
// reads outside the pool.  No waits, no atomics; a launch is at most slice_blocks compressions long.
namespace {
// one compression of the quad's message on block words m[16] (LDS); tb = t after this block
__device__ __forceinline__ void b2_quad_compress(uint64_t& h0, uint64_t& h1, const uint64_t* m, uint64_t iv0,
                                                 uint64_t iv1, int q, uint64_t tb, bool last, bool live) {
    const int sh = 4 * q;
    uint64_t mw[12][4];
#pragma unroll
    for (int r = 0; r < 12; r++) {
        mw[r][0] = m[(sigma_pack(r, 0) >> sh) & 15];
        mw[r][1] = m[(sigma_pack(r, 1) >> sh) & 15];
        mw[r][2] = m[(sigma_pack(r, 8) >> sh) & 15];
        mw[r][3] = m[(sigma_pack(r, 9) >> sh) & 15];
    }
    uint64_t va = h0, vb = h1, vc = iv0, vd = iv1;
    if (q == 0) vd ^= tb;
    if (q == 2 && last) vd = ~vd;
#pragma unroll
    for (int r = 0; r < 12; r++) {
        b2_g(va, vb, vc, vd, mw[r][0], mw[r][1]);
        vb = quad_rot<QP_NEXT1>(vb);
        vc = quad_rot<QP_NEXT2>(vc);
        vd = quad_rot<QP_NEXT3>(vd);
        b2_g(va, vb, vc, vd, mw[r][2], mw[r][3]);
        vb = quad_rot<QP_NEXT3>(vb);
        vc = quad_rot<QP_NEXT2>(vc);
        vd = quad_rot<QP_NEXT1>(vd);
    }
    if (live) {
        h0 ^= va ^ vc;
        h1 ^= vb ^ vd;
    }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(64) k_blake2b_slice(
    uint32_t nrec, const uint4* __restrict__ recs, const uint8_t* __restrict__ pool, uint32_t slice_blocks,
    uint32_t pool_chunks, uint32_t n_slots, uint64_t* __restrict__ state, uint32_t* __restrict__ out,
    uint32_t* __restrict__ out2) {
    __shared__ uint64_t blk[16][16];
    const int lane = threadIdx.x, q = lane & 3, sl = lane >> 2;
    const uint32_t i = blockIdx.x * 16 + sl;
    uint4 ra = make_uint4(0, 0, 0, 0), rb = ra;  // slot, chunk, first_block, nblocks | flags, last_len
    if (i < nrec) {
        ra = recs[2 * (size_t)i];
        rb = recs[2 * (size_t)i + 1];
    }
    const bool active = i < nrec && ra.x < n_slots && pool_chunks > 0;
    const uint32_t slot = active ? ra.x : 0;
    const uint32_t chunk = active ? (ra.y < pool_chunks ? ra.y : pool_chunks - 1) : 0;
    const uint32_t fb = ra.z < slice_blocks ? ra.z : slice_blocks;
    const uint32_t nb = active ? (ra.w < slice_blocks - fb ? ra.w : slice_blocks - fb) : 0;
    const bool first = (rb.x & 1u) != 0, fin = (rb.x & 2u) != 0;
    const uint32_t last_len = rb.y < 128u ? rb.y : 128u;
    uint32_t nmax = nb;  // blocks of the longest record of the wave
    for (int o = 4; o < 64; o <<= 1) {
        const uint32_t t = __shfl_xor(nmax, o);
        nmax = t > nmax ? t : nmax;
    }
    const uint64_t iv0 = iv64(q), iv1 = iv64(q + 4);
    uint64_t* st = state + 16 * (size_t)slot;
    uint64_t h0 = iv0, h1 = iv1, t = 0;
    if (q == 0) h0 ^= 0x01010000u ^ 32u;
    if (active && !first) {
        h0 = st[q];
        h1 = st[4 + q];
        t = st[8];
    }
    const uint4* p = reinterpret_cast<const uint4*>(pool + ((size_t)chunk * slice_blocks + fb) * 128 + 32 * q);
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
    if (nb > 0) {
        w0 = p[0];
        w1 = p[1];
    }
#pragma unroll 1
    for (uint32_t b = 0; b < nmax; b++) {
        const bool live = b < nb;
        blk[sl][4 * q + 0] = (uint64_t)w0.x | ((uint64_t)w0.y << 32);
        blk[sl][4 * q + 1] = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
        blk[sl][4 * q + 2] = (uint64_t)w1.x | ((uint64_t)w1.y << 32);
        blk[sl][4 * q + 3] = (uint64_t)w1.z | ((uint64_t)w1.w << 32);
        if (b + 1 < nb) {
            w0 = p[8 * (size_t)(b + 1)];
            w1 = p[8 * (size_t)(b + 1) + 1];
        }
        __syncthreads();
        const bool last = fin && b + 1 == nb;
        if (live) t += last ? last_len : 128u;
        b2_quad_compress(h0, h1, blk[sl], iv0, iv1, q, t, last, live);
        __syncthreads();
    }
    if (active) {
        st[q] = h0;
        st[4 + q] = h1;
        if (q == 0) st[8] = t;
        if (fin) {
            out[8 * (size_t)slot + 2 * q] = (uint32_t)h0;
            out[8 * (size_t)slot + 2 * q + 1] = (uint32_t)(h0 >> 32);
            out2[8 * (size_t)slot + 2 * q] = (uint32_t)h0;
            out2[8 * (size_t)slot + 2 * q + 1] = (uint32_t)(h0 >> 32);
        }
    }
}
