// Where the base-gradient kernels (cnf_basegrad.hip) keep their words inside the handle's one grow-only buffer.  Plain C++ (no
// HIP), so that tests/support/basegrad_plan_test.cpp can hold the layout to its rule on the CPU.
//   [ tickets ][ result: ntiles x BG_REC ][ partials: nchunks x ntiles x BG_REC ][ whitened rows: B x n_in ]
// (floats; tickets are unsigned words of the same size).  The ticket region is sized by the DENSE kind's tile count whatever
// the kind of the call: the kind of a handle's base may change between calls while the buffer is cleared only when it grows,
// so no word that one kind uses as a ticket (zero between launches) may ever hold another kind's result or partial.
// A record is one 16 x 16 tile of M (entry (r, c) at 16 r + c; the diagonal kind uses its first 16 floats for 16 diagonal
// entries), then the tile's 16 entries of m (tiles of block column 0 only), then sum_b w_b (tile 0 only).
#pragma once
#include <algorithm>
#include <cstddef>

constexpr int BG_REC = 288;
constexpr int BG_M = 256, BG_W = 272;           // offsets of m and of sum w inside a record
struct BaseGradPlan {
    int nt;                // 16-row blocks of n_in
    int ntiles;            // dense: nt (nt + 1) / 2 lower-triangular tiles, tile (ti, tj) at ti (ti + 1) / 2 + tj; diagonal: nt
    int chunk, nchunks;    // samples per workgroup (a multiple of 16) and workgroups along the batch
    size_t off_result, off_part, off_rows, floats;
};

inline BaseGradPlan base_grad_plan(int n_in, int kind, int B) {
    BaseGradPlan p{};
    p.nt = (n_in + 15) / 16;
    const int dense_tiles = p.nt * (p.nt + 1) / 2;
    p.ntiles = kind == 1 ? p.nt : dense_tiles;
    // at most 64 chunks of a multiple of 16 samples, 64 samples at least where the batch has them
    const int per = std::max(64, (B + 63) / 64);
    p.chunk = (std::min(per, std::max(B, 1)) + 15) & ~15;
    p.nchunks = (std::max(B, 1) + p.chunk - 1) / p.chunk;
    p.off_result = ((size_t)dense_tiles + 63) & ~(size_t)63;
    p.off_part = p.off_result + (size_t)p.ntiles * BG_REC;
    p.off_rows = p.off_part + (size_t)p.nchunks * p.ntiles * BG_REC;
    p.floats = p.off_rows + (size_t)B * n_in;
    return p;
}
