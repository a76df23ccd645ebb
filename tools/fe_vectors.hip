// fe_vectors.hip -- the device's fe_mul, fe_sq and fe_sqn on limb vectors from a file, one element
// per lane (tests/test_gpu_fe_seeded.py): the device path of fe25519.h's column sums is inline
// assembly the host emulation cannot run.
//   fe_vectors IN OUT
// IN:  uint32 n, uint32 nsq, then n x 10 limbs of a, then n x 10 limbs of b (little-endian words)
// OUT: n x 30 limbs: a b | a^2 | a^(2^nsq) per element
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../narwhal_amd/csrc/fe25519.h"

using namespace nwv;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

__global__ void __launch_bounds__(256) k_fe_vectors(uint32_t n, int nsq, const uint32_t* a, const uint32_t* b,
                                                    uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    fe f, g;
    for (int i = 0; i < 10; i++) f.v[i] = a[10 * (size_t)t + i], g.v[i] = b[10 * (size_t)t + i];
    const fe m = fe_mul(f, g), s = fe_sq(f), q = fe_sqn(f, nsq);
    uint32_t* o = out + 30 * (size_t)t;
    for (int i = 0; i < 10; i++) o[i] = m.v[i], o[10 + i] = s.v[i], o[20 + i] = q.v[i];
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: fe_vectors IN OUT\n");
        return 1;
    }
    FILE* fi = fopen(argv[1], "rb");
    uint32_t hdr[2];
    if (!fi || fread(hdr, 4, 2, fi) != 2 || hdr[0] == 0 || hdr[0] > (1u << 20) || hdr[1] > 4096) {
        fprintf(stderr, "fe_vectors: cannot read %s\n", argv[1]);
        return 1;
    }
    const uint32_t n = hdr[0];
    std::vector<uint32_t> ab(20 * (size_t)n), res(30 * (size_t)n);
    if (fread(ab.data(), 4, ab.size(), fi) != ab.size()) {
        fprintf(stderr, "fe_vectors: %s is short\n", argv[1]);
        return 1;
    }
    fclose(fi);
    uint32_t *da, *dout;
    CHECK(hipMalloc(&da, 4 * ab.size()));
    CHECK(hipMalloc(&dout, 4 * res.size()));
    CHECK(hipMemcpy(da, ab.data(), 4 * ab.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fe_vectors, dim3((n + 255) / 256), dim3(256), 0, 0, n, (int)hdr[1], da, da + 10 * (size_t)n, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(res.data(), dout, 4 * res.size(), hipMemcpyDeviceToHost));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo || fwrite(res.data(), 4, res.size(), fo) != res.size() || fclose(fo) != 0) {
        fprintf(stderr, "fe_vectors: cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}
