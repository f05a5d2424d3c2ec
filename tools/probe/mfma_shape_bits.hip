// Do 2 x v_mfma_f32_32x32x16_bf16 and 1 x v_mfma_f32_16x16x32_bf16 give the same f32 bits?  One wave forms the same 32 x 32 block of A[32][K] . B[32][K]^T
// on random bf16 operands both ways (K ascending in both) and the host compares the bits after 32 products per output and at the model's K = 768.
// build + run: hipcc --offload-arch=gfx950 -O3 tools/probe/mfma_shape_bits.hip -o mfma_shape_bits && ./mfma_shape_bits
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ __launch_bounds__(64) void k(const unsigned short* A, const unsigned short* B, int K, float* d32, float* d16) {
    const int l = threadIdx.x;
    f32x16 c32 = {};
    f32x4 c16[2][2] = {};
    for (int k0 = 0; k0 < K; k0 += 32) {
        for (int h = 0; h < 2; h++) {          // A = row-side operand (lane = row l & 31, k = 8 (l >> 5) ..), B = column side
            const bf16x8 a = *(const bf16x8*)(A + (l & 31) * K + k0 + 16 * h + 8 * (l >> 5)), b = *(const bf16x8*)(B + (l & 31) * K + k0 + 16 * h + 8 * (l >> 5));
            c32 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c32, 0, 0, 0);
        }
        for (int i = 0; i < 2; i++)            // lane = row / column l & 15, k = 8 (l >> 4) ..
            for (int j = 0; j < 2; j++) {
                const bf16x8 a = *(const bf16x8*)(A + (16 * i + (l & 15)) * K + k0 + 8 * (l >> 4)), b = *(const bf16x8*)(B + (16 * j + (l & 15)) * K + k0 + 8 * (l >> 4));
                c16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c16[i][j], 0, 0, 0);
            }
    }
    for (int r = 0; r < 16; r++) d32[((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = c32[r];
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            for (int r = 0; r < 4; r++) d16[(16 * i + 4 * (l >> 4) + r) * 32 + 16 * j + (l & 15)] = c16[i][j][r];
}

static unsigned short bf16_of(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }
static float f_of(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }

int main() {
    const int Ks[2] = {32, 768};
    for (int t = 0; t < 2; t++) {
        const int K = Ks[t];
        unsigned short *hA = (unsigned short*)malloc(32 * K * 2), *hB = (unsigned short*)malloc(32 * K * 2), *A, *B;
        srand(1234 + K);
        for (int i = 0; i < 32 * K; i++) {     // sums of twelve uniforms: near-normal, as activations / weights scaled by 1 / sqrt(K)
            float a = -6.f, b = -6.f;
            for (int q = 0; q < 12; q++) { a += rand() / (float)RAND_MAX; b += rand() / (float)RAND_MAX; }
            hA[i] = bf16_of(a); hB[i] = bf16_of(b / sqrtf((float)K));
        }
        float *d32, *d16, h32[1024], h16[1024];
        hipMalloc(&A, 32 * K * 2); hipMalloc(&B, 32 * K * 2); hipMalloc(&d32, 4096); hipMalloc(&d16, 4096);
        hipMemcpy(A, hA, 32 * K * 2, hipMemcpyHostToDevice); hipMemcpy(B, hB, 32 * K * 2, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, A, B, K, d32, d16);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
        hipMemcpy(h32, d32, 4096, hipMemcpyDeviceToHost); hipMemcpy(h16, d16, 4096, hipMemcpyDeviceToHost);
        int ndiff = 0; double maxd = 0, maxe32 = 0, maxe16 = 0;
        for (int i = 0; i < 32; i++)
            for (int j = 0; j < 32; j++) {
                double ref = 0;
                for (int kk = 0; kk < K; kk++) ref += (double)f_of(hA[i * K + kk]) * (double)f_of(hB[j * K + kk]);
                const float x = h32[i * 32 + j], y = h16[i * 32 + j];
                if (memcmp(&x, &y, 4)) ndiff++;
                maxd = fmax(maxd, fabs((double)x - y)); maxe32 = fmax(maxe32, fabs(x - ref)); maxe16 = fmax(maxe16, fabs(y - ref));
            }
        printf("K=%d: %d of 1024 outputs differ in bits, max |32x32x16 - 16x16x32| = %.3g; max |err| against float64: 32x32x16 %.3g, 16x16x32 %.3g\n", K, ndiff, maxd, maxe32, maxe16);
    }
    return 0;
}
