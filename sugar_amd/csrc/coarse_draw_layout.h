// coarse_draw_layout.h -- the scratch layout of csrc/coarse_draw.hip as plain host C++ (no HIP), as coarse_loss_layout.h:
//   ids u32[P] (the masked row numbers, ascending; the first n_masked entries are written) | block_off u32[ceil(P / 2048)]
// Every part starts 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum { CD_ROWS_PER_BLOCK = 2048 };   // 256 threads x 8 consecutive rows

struct CdLayout { size_t ids, block_off, total, n_blocks; };
static inline CdLayout cd_layout(int P)
{
    const size_t p = (size_t)(P > 0 ? P : 0);
    CdLayout L;
    L.n_blocks = (p + CD_ROWS_PER_BLOCK - 1) / CD_ROWS_PER_BLOCK;
    size_t off = 0;
    L.ids = off;       off = (off + p * sizeof(uint32_t) + 255) / 256 * 256;
    L.block_off = off; off = (off + L.n_blocks * sizeof(uint32_t) + 255) / 256 * 256;
    L.total = off > 256 ? off : 256;
    return L;
}
