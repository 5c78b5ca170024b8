// Micro-benchmark: what does a packed f32 VALU instruction (v_pk_mul_f32 / v_pk_add_f32) cost a wave on MI355X, against the two plain
// instructions it stands for -- for a wave that is alone on its SIMD (the solver's colour launches) and for four waves per SIMD?
//  1. bare runs (inline assembly): N independent / N dependent v_pk_mul_f32 and v_pk_add_f32 against 2N v_mul_f32 / v_add_f32;
//  2. one source function, a chain of v3 updates shaped like the solver's half_jv + half_apply (dot, dot, add, swap with the neighbour
//     lane, scale, subtract), compiled twice: with the SLP vectorizer (it pairs the f32 ops) and with -fno-slp-vectorize.
// One workgroup of 256 threads is one wave per SIMD of one CU, one of 1024 threads is four; every wave times itself with s_memtime.
// Build (three translation units of this one file):
//   F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math"
//   hipcc $F -DPK_CHAIN_TU=slp -c pk_f32_issue_bench.hip -o pk_chain_slp.o
//   hipcc $F -DPK_CHAIN_TU=scalar -fno-slp-vectorize -c pk_f32_issue_bench.hip -o pk_chain_scalar.o
//   hipcc $F -c pk_f32_issue_bench.hip -o pk_main.o
//   hipcc --offload-arch=gfx950 pk_main.o pk_chain_slp.o pk_chain_scalar.o -o pk_f32_issue_bench
// Run: ./pk_f32_issue_bench            (a second of GPU time; prints a markdown table)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>

#define CHAIN_ROWS 4                     // rows (axis, arm, inertia-scaled arm, effective mass) a lane cycles through, like a manifold's points
#define CHAIN_ROW_FLOATS 12              // axis.xyz c.xyz iv.xyz eff pad pad
#define CHAIN_STEPS 128                  // chain steps per measurement (a multiple of CHAIN_ROWS)

// wave-level timestamp: the shader clock, read when the scalar unit gets to it
#define PK_CLOCK(t) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory")

#ifdef PK_CHAIN_TU
// ---------------------------------------------------------------- the chain, one translation unit per flag set
#define PK_CAT2(a, b) a##b
#define PK_CAT(a, b) PK_CAT2(a, b)

namespace {
struct v3 { float x, y, z; };
__device__ inline v3 v3_add(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline v3 v3_sub(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline v3 v3_scale(v3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ inline float v3_dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline float lane_swap1(float x) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, true)); }

// (the solver's half_jv and half_apply, sgp_dev_solve.h)
__device__ inline float half_jv(v3 lv, v3 av, v3 axis, v3 c, int side)
{
	const float mine = v3_dot(axis, lv) + v3_dot(c, av);
	const float other = lane_swap1(mine);
	return side ? other - mine : mine - other;
}
__device__ inline void half_apply(v3& lv, v3& av, float im, v3 axis, v3 iv, float lambda, int side)
{
	if (side) { lv = v3_add(lv, v3_scale(axis, lambda * im)); av = v3_add(av, v3_scale(iv, lambda)); }
	else      { lv = v3_sub(lv, v3_scale(axis, lambda * im)); av = v3_sub(av, v3_scale(iv, lambda)); }
}
}

__global__ void __launch_bounds__(1024) PK_CAT(k_chain_, PK_CHAIN_TU)(const float* rows, float* out, unsigned long long* cycles)
{
	const int side = threadIdx.x & 1;
	v3 axis[CHAIN_ROWS], c[CHAIN_ROWS], iv[CHAIN_ROWS]; float eff[CHAIN_ROWS];
#pragma unroll
	for (int r = 0; r < CHAIN_ROWS; ++r) {
		const float* p = rows + r * CHAIN_ROW_FLOATS;
		axis[r] = {p[0], p[1], p[2]}; c[r] = {p[3], p[4], p[5]}; iv[r] = {p[6], p[7], p[8]}; eff[r] = p[9];
	}
	const float im = rows[CHAIN_ROWS * CHAIN_ROW_FLOATS];
	v3 lv = {0.5f + 0.001f * threadIdx.x, -0.25f, 0.125f}, av = {0.1f, 0.2f, -0.3f};
	unsigned long long t0, t1;
	PK_CLOCK(t0);
	asm volatile("" : "+v"(lv.x), "+v"(lv.y), "+v"(lv.z), "+v"(av.x), "+v"(av.y), "+v"(av.z));      // the chain starts after the first timestamp
	for (int s = 0; s < CHAIN_STEPS / CHAIN_ROWS; ++s) {
#pragma unroll
		for (int r = 0; r < CHAIN_ROWS; ++r) {
			const float lambda = eff[r] * half_jv(lv, av, axis[r], c[r], side);
			half_apply(lv, av, im, axis[r], iv[r], lambda, side);
		}
	}
	asm volatile("" :: "v"(lv.x), "v"(lv.y), "v"(lv.z), "v"(av.x), "v"(av.y), "v"(av.z));           // ... and ends before the second
	PK_CLOCK(t1);
	float* o = out + 6 * threadIdx.x;
	o[0] = lv.x; o[1] = lv.y; o[2] = lv.z; o[3] = av.x; o[4] = av.y; o[5] = av.z;
	if ((threadIdx.x & 63) == 0) cycles[threadIdx.x >> 6] = t1 - t0;
}

extern "C" void PK_CAT(launch_chain_, PK_CHAIN_TU)(const float* rows, float* out, unsigned long long* cycles, int threads, hipStream_t s)
{
	hipLaunchKernelGGL(PK_CAT(k_chain_, PK_CHAIN_TU), dim3(1), dim3(threads), 0, s, rows, out, cycles);
}

#else
// ---------------------------------------------------------------- the bare runs and main
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

extern "C" void launch_chain_slp(const float* rows, float* out, unsigned long long* cycles, int threads, hipStream_t s);
extern "C" void launch_chain_scalar(const float* rows, float* out, unsigned long long* cycles, int threads, hipStream_t s);

typedef float f2 __attribute__((ext_vector_type(2)));

#define BARE_N 4096                      // packed instructions per measurement (2 * BARE_N plain ones)
#define BARE_UNROLL 8                    // independent accumulators (pairs) of the independent runs

enum { PK_MUL_IND, PK_MUL_DEP, MUL_IND, MUL_DEP2, MUL_DEP1, PK_ADD_IND, PK_ADD_DEP, ADD_IND, ADD_DEP2, FMA_IND, PK_FMA_IND, BARE_KINDS };
static const char* const BARE_NAMES[BARE_KINDS] = {
	"N v_pk_mul_f32, independent (8 pairs in rotation)", "N v_pk_mul_f32, dependent (one pair)",
	"2N v_mul_f32, independent (16 registers in rotation)", "2N v_mul_f32, two interleaved dependent chains (= one dependent pair)", "2N v_mul_f32, one dependent chain",
	"N v_pk_add_f32, independent", "N v_pk_add_f32, dependent", "2N v_add_f32, independent", "2N v_add_f32, two interleaved dependent chains",
	"2N v_fma_f32, independent", "N v_pk_fma_f32, independent" };

template <int KIND> __global__ void __launch_bounds__(1024) k_bare(float* out, unsigned long long* cycles, float m_in)
{
	f2 a[BARE_UNROLL];
#pragma unroll
	for (int k = 0; k < BARE_UNROLL; ++k) a[k] = f2{1.0f + 0.001f * threadIdx.x, 1.0f + k};
	const float m1 = m_in;                 // 1.0 for the multiplies, 0.0 for the adds: the values stay where they are
	const f2 m = f2{m_in, m_in};
	unsigned long long t0, t1;
	PK_CLOCK(t0);
	for (int it = 0; it < BARE_N / (BARE_UNROLL * 8); ++it) {
#pragma unroll
		for (int u = 0; u < 8; ++u) {
#pragma unroll
			for (int k = 0; k < BARE_UNROLL; ++k) {
				f2& x = a[KIND == PK_MUL_DEP || KIND == PK_ADD_DEP || KIND == MUL_DEP2 || KIND == ADD_DEP2 || KIND == MUL_DEP1 ? 0 : k];
				if (KIND == PK_MUL_IND || KIND == PK_MUL_DEP) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(x) : "v"(m));
				else if (KIND == PK_ADD_IND || KIND == PK_ADD_DEP) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(x) : "v"(m));
				else if (KIND == PK_FMA_IND) asm volatile("v_pk_fma_f32 %0, %0, %1, %0" : "+v"(x) : "v"(m));
				else if (KIND == MUL_IND || KIND == MUL_DEP2) { asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x.x) : "v"(m1)); asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x.y) : "v"(m1)); }
				else if (KIND == MUL_DEP1) { asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x.x) : "v"(m1)); asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x.x) : "v"(m1)); }
				else if (KIND == ADD_IND || KIND == ADD_DEP2) { asm volatile("v_add_f32 %0, %0, %1" : "+v"(x.x) : "v"(m1)); asm volatile("v_add_f32 %0, %0, %1" : "+v"(x.y) : "v"(m1)); }
				else if (KIND == FMA_IND) { asm volatile("v_fma_f32 %0, %0, %1, %0" : "+v"(x.x) : "v"(m1)); asm volatile("v_fma_f32 %0, %0, %1, %0" : "+v"(x.y) : "v"(m1)); }
			}
		}
	}
	PK_CLOCK(t1);
	float acc = 0.0f;
#pragma unroll
	for (int k = 0; k < BARE_UNROLL; ++k) acc += a[k].x + a[k].y;
	out[threadIdx.x] = acc;
	if ((threadIdx.x & 63) == 0) cycles[threadIdx.x >> 6] = t1 - t0;
}

struct Buf { float* rows; float* out; unsigned long long* cycles; };

// median over the waves of the workgroup of the best of `reps` launches
template <class L> static int measure(L launch, const Buf& b, int threads, double& cyc)
{
	const int waves = threads / 64;
	std::vector<unsigned long long> best(waves, ~0ull), h(waves);
	for (int rep = 0; rep < 5; ++rep) {
		launch(threads);
		CHECK(hipDeviceSynchronize());
		CHECK(hipMemcpy(h.data(), b.cycles, waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		for (int w = 0; w < waves; ++w) best[w] = std::min(best[w], h[w]);
	}
	std::sort(best.begin(), best.end());
	cyc = (double)best[waves / 2];
	return 0;
}

template <int KIND> static int bare(const Buf& b)
{
	const float m = (KIND == PK_ADD_IND || KIND == PK_ADD_DEP || KIND == ADD_IND || KIND == ADD_DEP2 || KIND == FMA_IND || KIND == PK_FMA_IND) ? 0.0f : 1.0f;
	double c1, c4;
	if (measure([&](int t) { hipLaunchKernelGGL((k_bare<KIND>), dim3(1), dim3(t), 0, 0, b.out, b.cycles, m); }, b, 256, c1)) return 1;
	if (measure([&](int t) { hipLaunchKernelGGL((k_bare<KIND>), dim3(1), dim3(t), 0, 0, b.out, b.cycles, m); }, b, 1024, c4)) return 1;
	const bool packed = KIND == PK_MUL_IND || KIND == PK_MUL_DEP || KIND == PK_ADD_IND || KIND == PK_ADD_DEP || KIND == PK_FMA_IND;
	const double n = packed ? BARE_N : 2.0 * BARE_N;
	// per instruction as the wave sees it, and (four waves) per instruction of the SIMD's stream
	printf("| %s | %.0f | %.2f | %.2f | %.0f | %.2f | %.2f |\n", BARE_NAMES[KIND], c1, c1 / n, c1 / BARE_N, c4, c4 / n / 4.0, c4 / BARE_N / 4.0);
	return 0;
}

int main()
{
	Buf b;
	CHECK(hipMalloc(&b.rows, (CHAIN_ROWS * CHAIN_ROW_FLOATS + 4) * sizeof(float)));
	CHECK(hipMalloc(&b.out, 1024 * 6 * sizeof(float)));
	CHECK(hipMalloc(&b.cycles, 16 * sizeof(unsigned long long)));
	std::vector<float> rows(CHAIN_ROWS * CHAIN_ROW_FLOATS + 4, 0.0f);
	const float ax[CHAIN_ROWS][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.6f, 0.8f, 0}};
	for (int r = 0; r < CHAIN_ROWS; ++r) {
		float* p = &rows[r * CHAIN_ROW_FLOATS];
		for (int k = 0; k < 3; ++k) { p[k] = ax[r][k]; p[3 + k] = 0.25f * ax[(r + 1) % CHAIN_ROWS][k]; p[6 + k] = 0.5f * p[3 + k]; }
		p[9] = 0.2f;      // effective mass: the chain contracts, values stay finite and normal
	}
	rows[CHAIN_ROWS * CHAIN_ROW_FLOATS] = 1.0f;      // inverse mass
	CHECK(hipMemcpy(b.rows, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
	hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
	printf("device: %s, shader clock %d MHz; one workgroup: 256 threads = 1 wave/SIMD, 1024 threads = 4 waves/SIMD; cycles are s_memtime ticks, median wave of the best of 5 launches\n\n", prop.gcnArchName, prop.clockRate / 1000);

	printf("bare runs, N = %d\n\n", BARE_N);
	printf("| run | 1 wave/SIMD: cycles | per instruction | per pair of f32 ops | 4 waves/SIMD: cycles | per instruction of the SIMD | per pair of the SIMD |\n|---|---|---|---|---|---|---|\n");
	if (bare<PK_MUL_IND>(b) || bare<PK_MUL_DEP>(b) || bare<MUL_IND>(b) || bare<MUL_DEP2>(b) || bare<MUL_DEP1>(b)) return 1;
	if (bare<PK_ADD_IND>(b) || bare<PK_ADD_DEP>(b) || bare<ADD_IND>(b) || bare<ADD_DEP2>(b)) return 1;
	if (bare<FMA_IND>(b) || bare<PK_FMA_IND>(b)) return 1;

	printf("\nchain of %d half_jv + half_apply steps, one source, two builds\n\n", CHAIN_STEPS);
	printf("| build | 1 wave/SIMD: cycles | per chain step | 4 waves/SIMD: cycles | per chain step of the SIMD |\n|---|---|---|---|---|\n");
	std::vector<float> ref(1024 * 6), got(1024 * 6);
	for (int v = 0; v < 2; ++v) {
		double c1, c4;
		auto launch = [&](int t) { (v ? launch_chain_scalar : launch_chain_slp)(b.rows, b.out, b.cycles, t, 0); };
		if (measure(launch, b, 256, c1) || measure(launch, b, 1024, c4)) return 1;
		CHECK(hipMemcpy((v ? got : ref).data(), b.out, 1024 * 6 * sizeof(float), hipMemcpyDeviceToHost));
		printf("| %s | %.0f | %.1f | %.0f | %.1f |\n", v ? "-fno-slp-vectorize" : "-O3 (SLP pairs the f32 ops)", c1, c1 / CHAIN_STEPS, c4, c4 / CHAIN_STEPS / 4.0);
	}
	printf("\nchain results of the two builds bit-identical: %s\n", std::memcmp(ref.data(), got.data(), ref.size() * sizeof(float)) == 0 ? "yes" : "NO");
	return 0;
}
#endif
