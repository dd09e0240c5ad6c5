// TEST INFRASTRUCTURE: a host program of its own over sugar_amd/csrc/coarse_loss_layout.h, the scratch layouts of csrc/coarse_loss.hip.
// For a set of shapes it allocates a heap block of EXACTLY the reported size, carves it as the entry points do and writes every part
// end to end, then checks alignment, order and that the parts do not overlap.  tests/test_coarse_loss_cpu.py builds and runs it plain;
// the sanitizer run is this same file with the sanitizers switched on, host code only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isugar_amd/csrc
//         tests/host/coarse_loss_layout_main.cpp -o coarse_loss_layout   (one command line)   and then   ./coarse_loss_layout
//
// (an out-of-bounds write of a part, a size that wraps, or a misaligned 8-byte store ends the program there).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coarse_loss_layout.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// the grouping's scratch (csrc/group.hip) is opaque here: any size, the layout only has to reserve it
static size_t fake_group_bytes(size_t entries) { return entries * 4 * 4 + 4096 + 17; }

static void estimation(long long N)
{
    const size_t nb = cl_estimation_blocks(N), bytes = cl_estimation_scratch_bytes(N);
    CHECK(nb * 256 >= (size_t)N && (nb == 0 || (nb - 1) * 256 < (size_t)N));
    CHECK(bytes % 256 == 0 && bytes >= 3 * nb * sizeof(double));
    std::vector<char> block(bytes);
    double* partial = reinterpret_cast<double*>(block.data());
    for (int row = 0; row < 3; row++)
        for (size_t b = 0; b < nb; b++) partial[(size_t)row * nb + b] = (double)row;     // as k_estimation_fwd writes them
}

static void normal_forward(long long N, int K)
{
    const size_t nb = cl_normal_blocks(N, K), bytes = cl_normal_fwd_scratch_bytes(N, K);
    const size_t per = K == 16 ? 16 : 256;
    CHECK(nb * per >= (size_t)N && (nb == 0 || (nb - 1) * per < (size_t)N));
    CHECK(bytes % 256 == 0 && bytes >= nb * sizeof(double));
    std::vector<char> block(bytes);
    double* partial = reinterpret_cast<double*>(block.data());
    for (size_t b = 0; b < nb; b++) partial[b] = 1.0;
}

static void normal_backward(long long N, int K, int P, int width)
{
    size_t entries = 0;
    CHECK(cl_normal_entries(N, K, &entries));
    CHECK(entries == (size_t)N * (size_t)(K + 1));
    const size_t group = fake_group_bytes(entries);
    const ClNormalBwdLayout L = cl_normal_bwd_layout(entries, P, width, group);
    CHECK(L.keys == 0 && L.keys % 256 == 0 && L.start % 256 == 0 && L.rows % 256 == 0 && L.group % 256 == 0 && L.total % 256 == 0);
    CHECK(L.keys + entries * 8 <= L.start);
    CHECK(L.start + ((size_t)P + 1) * 4 <= L.rows);
    CHECK(L.rows + entries * (size_t)width * 4 <= L.group);
    CHECK(L.group + group <= L.total);
    char* block = static_cast<char*>(std::malloc(L.total));       // exactly the reported size: one byte past it is the sanitizer's
    CHECK(block != nullptr);
    if (!block) return;
    int64_t* keys = reinterpret_cast<int64_t*>(block + L.keys);
    uint32_t* start = reinterpret_cast<uint32_t*>(block + L.start);
    float* rows = reinterpret_cast<float*>(block + L.rows);
    for (size_t e = 0; e < entries; e++) keys[e] = (int64_t)e;
    for (size_t p = 0; p <= (size_t)P; p++) start[p] = (uint32_t)p;
    for (size_t e = 0; e < entries * (size_t)width; e++) rows[e] = 1.f;
    std::memset(block + L.group, 0x5a, group);
    CHECK(keys[entries - 1] == (int64_t)(entries - 1) && start[P] == (uint32_t)P && rows[entries * (size_t)width - 1] == 1.f);
    std::free(block);
}

int main()
{
    const long long Ns[] = {1, 15, 16, 17, 255, 256, 257, 4097, 6000, 20001};
    for (long long N : Ns) {
        estimation(N);
        for (int K : {1, 8, 16, 17}) {
            normal_forward(N, K);
            for (int P : {1, 2, 2500}) {
                normal_backward(N, K, P, 3);
                normal_backward(N, K, P, 6);
            }
        }
    }
    CHECK(cl_estimation_blocks(0) == 0 && cl_estimation_blocks(-5) == 0 && cl_estimation_scratch_bytes(0) == 0);
    // the 32-bit entry numbers of the grouping: N * (K + 1) must stay below 2^32, and nothing may wrap on the way
    size_t e = 0;
    CHECK(cl_normal_entries(252645135LL, 16, &e) && e == 4294967295ull);                  // 2^32 - 1 = 17 * 252645135
    CHECK(!cl_normal_entries(252645136LL, 16, &e));
    CHECK(!cl_normal_entries(4294967296LL, 1, &e) && !cl_normal_entries(0x7fffffffffffffffLL, 16, &e));
    CHECK(!cl_normal_entries(-1, 16, &e) && !cl_normal_entries(5, 0, &e));
    CHECK(cl_normal_entries(0, 16, &e) && e == 0);
    // sizes at the trainer's scale stay exact in size_t
    const ClNormalBwdLayout big = cl_normal_bwd_layout(17000000u, 2000000, 6, fake_group_bytes(17000000u));
    CHECK(big.rows - big.start >= 2000001u * 4u && big.group - big.rows >= 17000000ull * 24ull);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("layouts ok\n");
    return 0;
}
