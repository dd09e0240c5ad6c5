// coarse_draw.hip -- the random draws of SuGaR.sample_points_in_gaussians for the coarse stage's default call
// (sugar_scene/sugar_model.py:900-926 with a mask and `probabilities_proportional_to_volume=False`): every sample picks one Gaussian
// uniformly among the masked ones and takes three standard normals.  The torch statements it stands for -- `torch.multinomial` over a
// constant vector, `arange(P)[mask][idx]` (a boolean-mask index: `nonzero` and a host wait) and `randn_like` -- become four launches
// and no host read:
//
//   k_mask_count   : every workgroup counts the set bytes of its 2048 rows of the mask
//   k_mask_offsets : ONE workgroup turns the counts into exclusive offsets (a running carry over chunks of 256) and writes n_masked
//   k_mask_compact : every workgroup writes the row numbers of its set bytes, ascending, behind its offset (sgr_block_scan)
//   k_draw         : one lane per sample: two Philox4x32-10 blocks, one 4-byte gather, 20 bytes written
//
// The stream is stated in include/sugar_raster.h (sgr_draw_samples) and restated bit for bit in tests/coarse_draw_restatement.py: the
// indices are pinned exactly, the normals (accurate logf / sincosf, every operation rounded on its own: built with -ffp-contract=off)
// within the float32 yard.
#include "../../include/sugar_raster.h"
#include "coarse_draw_layout.h"
#include "sgr_device.h"

namespace {

constexpr int DRAW_ITEMS = CD_ROWS_PER_BLOCK / 256;   // consecutive rows per thread

// the first row of this thread's DRAW_ITEMS consecutive rows (may lie at or beyond P: rows_set then reads nothing)
__device__ __forceinline__ long long first_row() { return ((long long)blockIdx.x * 256 + threadIdx.x) * DRAW_ITEMS; }

__device__ __forceinline__ uint32_t rows_set(const uint8_t* __restrict__ mask, int P, long long base, uint32_t& bits)
{
    uint32_t n = 0;
    bits = 0;
#pragma unroll
    for (int i = 0; i < DRAW_ITEMS; i++) {
        const long long r = base + i;
        if (r < (long long)P && mask[r]) { bits |= 1u << i; n++; }
    }
    return n;
}

__global__ void __launch_bounds__(256) k_mask_count(int P, const uint8_t* __restrict__ mask, uint32_t* __restrict__ block_count)
{
    __shared__ uint32_t s_wave[4];
    uint32_t bits, excl;
    const uint32_t total = sgr_block_scan<4>(rows_set(mask, P, first_row(), bits), s_wave, excl);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// in place: block_count[b] becomes the number of set rows before workgroup b; the total goes to n_masked
__global__ void __launch_bounds__(256) k_mask_offsets(uint32_t n_blocks, uint32_t* __restrict__ block_count, long long* __restrict__ n_masked)
{
    __shared__ uint32_t s_wave[4];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 256) {                      // (uniform trip count: every thread reaches the barriers)
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_blocks ? block_count[b] : 0u;
        uint32_t excl;
        const uint32_t total = sgr_block_scan<4>(v, s_wave, excl);
        if (b < n_blocks) block_count[b] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) n_masked[0] = (long long)carry;
}

__global__ void __launch_bounds__(256) k_mask_compact(int P, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ block_off,
                                                      uint32_t* __restrict__ ids)
{
    __shared__ uint32_t s_wave[4];
    uint32_t bits, excl;
    const long long base = first_row();
    sgr_block_scan<4>(rows_set(mask, P, base, bits), s_wave, excl);
    uint32_t at = block_off[blockIdx.x] + excl;                            // < n_masked <= P: inside ids[P]
#pragma unroll
    for (int i = 0; i < DRAW_ITEMS; i++)
        if (bits & (1u << i)) ids[at++] = (uint32_t)(base + i);
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the standard constants
struct Philox { uint32_t r[4]; };
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

// u = ((r >> 8) + 0.5) 2^-24 in float32: never 0; the sum rounds to even once r >> 8 needs all 24 bits, so u may be exactly 1
__device__ __forceinline__ float unit_open(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f; }

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z_cos, float& z_sin)
{
    const float rho = sqrtf(-2.0f * logf(unit_open(ra)));
    const float theta = 6.283185307179586f * unit_open(rb);
    float s, c;
    sincosf(theta, &s, &c);
    z_cos = rho * c; z_sin = rho * s;
}

__global__ void __launch_bounds__(256) k_draw(long long N, const uint32_t* __restrict__ ids, const long long* __restrict__ n_masked,
                                              uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi,
                                              long long* __restrict__ sample_idx, float* __restrict__ noise)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const unsigned long long nm = (unsigned long long)n_masked[0];
    long long pick = 0;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f, unused;
    if (nm > 0) {
        const unsigned long long c = 2ull * (unsigned long long)n;
        const Philox a = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), call_lo, call_hi, seed_lo, seed_hi);
        const Philox b = philox4x32_10((uint32_t)(c + 1), (uint32_t)((c + 1) >> 32), call_lo, call_hi, seed_lo, seed_hi);
        pick = (long long)ids[((unsigned long long)a.r[0] * nm) >> 32];    // j < n_masked
        box_muller(a.r[1], a.r[2], z0, z1);
        box_muller(b.r[0], b.r[1], z2, unused);
    }
    sample_idx[n] = pick;
    noise[3 * n] = z0; noise[3 * n + 1] = z1; noise[3 * n + 2] = z2;
}

}  // namespace

extern "C" {

size_t sgr_draw_samples_scratch_bytes(int P) { return cd_layout(P).total; }

int sgr_draw_samples(int P, const uint8_t* mask, long long N, uint64_t seed, uint64_t call, int64_t* sample_idx, float* noise,
                     int64_t* n_masked, char* scratch, void* stream)
{
    if (P <= 0 || N < 0 || (unsigned long long)N > 0xFFFFFFFFull || !mask || !n_masked || !scratch || (N > 0 && (!sample_idx || !noise)))
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const CdLayout L = cd_layout(P);
    uint32_t* ids = reinterpret_cast<uint32_t*>(scratch + L.ids);
    uint32_t* block_off = reinterpret_cast<uint32_t*>(scratch + L.block_off);
    long long* nm = reinterpret_cast<long long*>(n_masked);
    const unsigned nb = (unsigned)L.n_blocks;
    hipLaunchKernelGGL(k_mask_count, dim3(nb), dim3(256), 0, s, P, mask, block_off);
    hipLaunchKernelGGL(k_mask_offsets, dim3(1), dim3(256), 0, s, (uint32_t)nb, block_off, nm);
    hipLaunchKernelGGL(k_mask_compact, dim3(nb), dim3(256), 0, s, P, mask, block_off, ids);
    if (N > 0)
        hipLaunchKernelGGL(k_draw, dim3(blocks256((size_t)N)), dim3(256), 0, s, N, ids, nm, (uint32_t)seed, (uint32_t)(seed >> 32),
                           (uint32_t)call, (uint32_t)(call >> 32), reinterpret_cast<long long*>(sample_idx), noise);
    return sgr_launch_status();
}

}  // extern "C"
