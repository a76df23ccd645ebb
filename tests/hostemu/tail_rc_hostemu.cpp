// tail_rc_hostemu.cpp -- TEST-ONLY host build (NWV_BOUNDS_CHECK: limb bounds and column sums below
// 2^63 asserted) of the chunk phase of k_msm_tail: the bit planes of C = 2^m bucket sums by rows
// and columns (msm.h tail_rc_op, run level by level as the workgroup runs it: every operation of
// a level reads the slots as the level found them, which is what the kernel's barriers give at
// level 0 and what the disjoint slots give afterwards -- checked here) against the one-butterfly
// form the kernel had before, and against sum (t + 1) S_t added up directly.  Never part of the product.
#define NWV_HD __host__ __device__ inline
#include <cstring>
#include <vector>

#include "../../narwhal_amd/csrc/msm.h"

using namespace nwv;

namespace {

bool frozen_eq(const fe& a, const fe& b) {
    uint32_t x[8], y[8];
    fe_freeze(a, x);
    fe_freeze(b, y);
    return std::memcmp(x, y, sizeof x) == 0;
}
// the same point: X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1, and each T consistent (T Z = X Y)
bool same_point(const ge_p3& a, const ge_p3& b) {
    return frozen_eq(fe_mul(a.X, b.Z), fe_mul(b.X, a.Z)) && frozen_eq(fe_mul(a.Y, b.Z), fe_mul(b.Y, a.Z)) &&
           frozen_eq(fe_mul(a.T, a.Z), fe_mul(a.X, a.Y)) && frozen_eq(fe_mul(b.T, b.Z), fe_mul(b.X, b.Y));
}

// the butterfly of the kernel's C <= 128 branch: slot 0 -> the sum, slot 2^k -> plane k
void butterfly(std::vector<ge_p3>& s, int C) {
    for (int o = 1, lg = 0; o < C; o <<= 1, lg++)
        for (int t = 0; t < C / 2; t++) {
            const int i = ((t >> lg) << (lg + 1)) | (t & (o - 1));
            s[i] = p3_add(s[i], s[i + o]);
        }
}

}  // namespace

extern "C" {

// enc: C = 2^m compressed points, bucket t's sum S_t.  Returns 0, or a mask: 1 a point does not
// decode; 2 an operation's slot is outside [0, C), or two operations of a level write one slot, or
// (after level 0) one reads a slot another writes at that level, or a level has more than 256
// operations; 4 a plane differs from the butterfly's; 8 the chunk's sum differs from the
// butterfly's; 16 sum_k 2^k T_k + U of the new planes differs from sum (t + 1) S_t added up
// directly.  info: [0] additions, [1] waves of additions (64 operations a wave, a level at a
// time), [2] the first differing plane or -1, [3] the largest operation count of a level.
int he_tail_rc_check(int m, const uint8_t* enc, int* info) {
    const int C = 1 << m;
    std::vector<ge_p3> raw(C);
    for (int t = 0; t < C; t++) {
        uint32_t w[8];
        std::memcpy(w, enc + 32 * (size_t)t, 32);
        if (!ge_decompress(w, raw[t])) return 1;
    }
    int rc = 0;
    info[0] = info[1] = info[3] = 0;
    info[2] = -1;
    std::vector<ge_p3> s = raw;
    for (int ph = 0; ph < m; ph++) {
        std::vector<TailRcOp> ops;
        for (int g = 0; g < 256; g++) {  // the workgroup's lanes
            TailRcOp op;
            if (tail_rc_op(m, ph, g, op)) ops.push_back(op);
        }
        TailRcOp extra;
        if (tail_rc_op(m, ph, 256, extra)) rc |= 2;
        std::vector<int> writes(C, 0);
        for (const TailRcOp& op : ops) {
            if (op.d < 0 || op.d >= C || op.a < 0 || op.a >= C || op.b < 0 || op.b >= C) return rc | 2;
            writes[op.d]++;
        }
        for (const TailRcOp& op : ops) {
            if (writes[op.d] != 1) rc |= 2;
            if (ph > 0 && ((op.a != op.d && writes[op.a]) || (op.b != op.d && writes[op.b]))) rc |= 2;
        }
        std::vector<ge_p3> res(ops.size());
        for (size_t k = 0; k < ops.size(); k++) res[k] = p3_add(s[ops[k].a], s[ops[k].b]);
        for (size_t k = 0; k < ops.size(); k++) s[ops[k].d] = res[k];
        info[0] += (int)ops.size();
        info[1] += ((int)ops.size() + 63) / 64;
        if ((int)ops.size() > info[3]) info[3] = (int)ops.size();
    }
    std::vector<ge_p3> bf = raw;
    butterfly(bf, C);
    for (int k = m - 1; k >= 0; k--)
        if (!same_point(s[tail_rc_plane_slot(m, k)], bf[1 << k])) {
            rc |= 4;
            info[2] = k;
        }
    if (!same_point(s[tail_rc_plane_slot(m, m)], bf[0])) rc |= 8;
    // sum (t + 1) S_t: running sums from the top bucket down
    ge_p3 run = ge_p3_identity(), want = ge_p3_identity();
    for (int t = C - 1; t >= 0; t--) {
        run = p3_add(run, raw[t]);
        want = p3_add(want, run);
    }
    ge_p3 got = ge_p3_identity();  // Horner over the planes, then the sum of all buckets
    for (int k = m - 1; k >= 0; k--) got = p3_add(p3_dbl_n(got, 1), s[tail_rc_plane_slot(m, k)]);
    got = p3_add(got, s[tail_rc_plane_slot(m, m)]);
    if (!same_point(got, want)) rc |= 16;
    return rc;
}

// msm_plan's entries per bucket lane (msm.h msm_bucket_seg)
uint32_t he_msm_bucket_seg(uint64_t n, uint64_t entries, uint32_t chunks) { return msm_bucket_seg(n, entries, chunks); }

}  // extern "C"
