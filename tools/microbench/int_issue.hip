// Integer address arithmetic on gfx950: issue cycles per wave instruction (8 independent chains) and dependent latency (one chain) of
// v_mul_lo_u32, v_mul_hi_u32, v_mul_u32_u24, v_mad_u32_u24, v_lshl_add_u32 and s_mul_i32 -> v_add_u32, at one and at two waves per
// SIMD (4 and 8 waves on one CU), and the G[W,:] sweep chunk of the active-set finish (8 x (row * gs, shift-add, ds_read_b128) + 16
// FMAs in two chains) with the multiplies and with offsets stored ready-made.  s_memtime based, cycles of wave 0.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/int_issue tools/microbench/int_issue.hip && /tmp/int_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { if ((x) != hipSuccess) { printf("HIP error at line %d\n", __LINE__); exit(1); } } while (0)
typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i4 __attribute__((ext_vector_type(4)));

constexpr int LINKS = 512;     // instructions per chain
constexpr int GROWS = 64, GS = 66;   // the chunk's matrix in LDS: 64 rows of stride 66 doubles (33 KB)

// (unrolled by hand: the optimiser leaves a loop around a single asm statement alone, and a taken branch per link would be measured)
#define R4(X) X X X X
#define R16(X) R4(R4(X))
#define ONE(INS, J) asm volatile(INS : "+v"(x[J]) : "v"(y));
#define ALL8(INS) ONE(INS, 0) ONE(INS, 1) ONE(INS, 2) ONE(INS, 3) ONE(INS, 4) ONE(INS, 5) ONE(INS, 6) ONE(INS, 7)
#define DEP1(INS) _Pragma("unroll 1") for (int i = 0; i < LINKS / 16; ++i) { R16(ONE(INS, 0)) }
#define IND8(INS) _Pragma("unroll 1") for (int i = 0; i < LINKS / 4; ++i) { R4(ALL8(INS)) }
#define SPAIR(J) asm volatile("s_mul_i32 %1, %1, %2\n\tv_add_u32 %0, %1, %0" : "+v"(x[J]), "+s"(sx) : "s"(sy));

// mode = 2 * instruction + (0: one dependent chain, 1: eight independent chains); 12, 13: the chunk with / without multiplies
__global__ __launch_bounds__(512) void k(int mode, int gs, unsigned seed, unsigned* out, long long* cyc, double* outd) {
    extern __shared__ __attribute__((aligned(16))) double G[];   // [GROWS * GS], dynamic as in the step kernels
    __shared__ __attribute__((aligned(16))) int idx[2][64];
    __shared__ __attribute__((aligned(16))) double wgt[64];
    const int lane = threadIdx.x & 63;
    for (int t = threadIdx.x; t < GROWS * GS; t += blockDim.x) G[t] = 1.0 + 1e-9 * t;
    if (threadIdx.x < 64) {
        const int row = (threadIdx.x * 7) & 63;
        idx[0][threadIdx.x] = row;         // row numbers
        idx[1][threadIdx.x] = row * gs;    // element offsets
        wgt[threadIdx.x] = 1.0 / (1 + threadIdx.x);
    }
    __syncthreads();
    unsigned x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = seed + lane + j;
    unsigned y = seed | 3u;
    int sx = __builtin_amdgcn_readfirstlane((int)seed), sy = __builtin_amdgcn_readfirstlane((int)(seed | 5u));
    double q0 = 0.0, q1 = 0.0;
    const int rc = 2 * (lane & 31), gse = gs & ~1;
    const long long t0 = __builtin_readcyclecounter();
    switch (mode) {
        case 0: DEP1("v_mul_lo_u32 %0, %0, %1"); break;
        case 1: IND8("v_mul_lo_u32 %0, %0, %1"); break;
        case 2: DEP1("v_mul_hi_u32 %0, %0, %1"); break;
        case 3: IND8("v_mul_hi_u32 %0, %0, %1"); break;
        case 4: DEP1("v_mul_u32_u24 %0, %0, %1"); break;
        case 5: IND8("v_mul_u32_u24 %0, %0, %1"); break;
        case 6: DEP1("v_mad_u32_u24 %0, %0, %1, %1"); break;
        case 7: IND8("v_mad_u32_u24 %0, %0, %1, %1"); break;
        case 8: DEP1("v_lshl_add_u32 %0, %0, 3, %1"); break;
        case 9: IND8("v_lshl_add_u32 %0, %0, 3, %1"); break;
        case 10:   // s_mul_i32 -> v_add_u32 reading its result: the scalar product is needed by the very next vector instruction
#pragma unroll 1
            for (int i = 0; i < LINKS / 16; ++i) { R16(SPAIR(0)) }
            break;
        case 11:   // the same pair, eight vector chains: issue cost of the pair
#pragma unroll 1
            for (int i = 0; i < LINKS / 4; ++i) { R4(SPAIR(0) SPAIR(1) SPAIR(2) SPAIR(3) SPAIR(4) SPAIR(5) SPAIR(6) SPAIR(7)) }
            break;
        case 12: case 13: {   // one link = one chunk of the sweep; indices of the chunk from LDS as the finish reads them
            const bool offs = mode == 13;
#pragma unroll 2
            for (int i = 0; i < LINKS; ++i) {
                const int l0 = (i & 7) * 8;
                int rows[8];
                const int* ib = idx[offs ? 1 : 0] + l0;
                const i4 a = *reinterpret_cast<const i4*>(ib), b = *reinterpret_cast<const i4*>(ib + 4);
                rows[0] = a[0]; rows[1] = a[1]; rows[2] = a[2]; rows[3] = a[3]; rows[4] = b[0]; rows[5] = b[1]; rows[6] = b[2]; rows[7] = b[3];
                d2 g[8];
                // (the finish knows gs to be even: without that knowledge here the 16-byte reads come out as ds_read2_b64)
                if (offs) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) { __builtin_assume((rows[t] & 1) == 0); g[t] = *reinterpret_cast<const d2*>(G + (rows[t] + rc)); }
                } else {
#pragma unroll
                    for (int t = 0; t < 8; ++t) g[t] = *reinterpret_cast<const d2*>(G + (rows[t] * gse + rc));
                }
                double av[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) av[t] = wgt[l0 + t];
#pragma unroll
                for (int t = 0; t < 8; ++t) { q0 += g[t][0] * av[t]; q1 += g[t][1] * av[t]; }
            }
        } break;
        default: break;
    }
    const long long t1 = __builtin_readcyclecounter();
    unsigned r = (unsigned)sx;
#pragma unroll
    for (int j = 0; j < 8; ++j) r ^= x[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
    outd[blockIdx.x * blockDim.x + threadIdx.x] = q0 + q1;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

int main() {
    unsigned* out; long long* cyc; double* outd;
    CHECK(hipMalloc(&out, 4 * 512)); CHECK(hipMalloc(&cyc, 8 * 8)); CHECK(hipMalloc(&outd, 8 * 512));
    const char* names[] = {"v_mul_lo_u32", "v_mul_hi_u32", "v_mul_u32_u24", "v_mad_u32_u24", "v_lshl_add_u32", "s_mul_i32 + v_add_u32"};
    const int wl[] = {1, 4, 8};   // waves on the CU: one alone, one per SIMD, two per SIMD
    printf("%-24s %-8s %14s %14s\n", "instruction", "waves", "dependent", "issue (8 ind.)");
    for (int ins = 0; ins < 6; ++ins)
        for (int waves : wl) {
            double c[2];
            for (int v = 0; v < 2; ++v) {
                long long h = 0;
                for (int rep = 0; rep < 2; ++rep) { hipLaunchKernelGGL(k, dim3(1), dim3(64 * waves), GROWS * GS * 8, 0, 2 * ins + v, GS, 12345u, out, cyc, outd); CHECK(hipDeviceSynchronize()); }
                CHECK(hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost));
                c[v] = (double)h / LINKS / (v ? 8 : 1);
            }
            printf("%-24s %-8d %14.2f %14.2f\n", names[ins], waves, c[0], c[1]);
        }
    printf("\nsweep chunk: 2 index reads, 8 x (address, ds_read_b128), 8 weight reads, 16 FMA in two chains; cycles per chunk\n");
    printf("%-8s %16s %16s\n", "waves", "row * gs", "offsets");
    for (int waves : wl) {
        double c[2];
        for (int v = 0; v < 2; ++v) {
            long long h = 0;
            for (int rep = 0; rep < 2; ++rep) { hipLaunchKernelGGL(k, dim3(1), dim3(64 * waves), GROWS * GS * 8, 0, 12 + v, GS, 12345u, out, cyc, outd); CHECK(hipDeviceSynchronize()); }
            CHECK(hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost));
            c[v] = (double)h / LINKS;
        }
        printf("%-8d %16.1f %16.1f\n", waves, c[0], c[1]);
    }
    return 0;
}
