// pt_tile.h — the adaptive calls' device side: the tile pass (pt_kernels_tile.hip: the megakernel's bodies compiled for
// TileParams) and the class selection, a step's evaluation and the resolve (pt_adaptive.hip).  Translation units of their own: pt_kernels.s, and so
// pt_kernel_isa_hash(), describes the frame kernels only.
//
// A call's band is whole image rows; a tile covers `tile` columns by `tile` rows of it, counted from the band's first row and
// column 0, tile t at tile column t % tiles_x and tile row t / tiles_x.  The OPEN-TILE LIST holds the ids of the tiles that still
// take samples; slot i of it owns the entries [i * tile^2, (i + 1) * tile^2) of the compact accumulator ([3] colour planes of
// slots * tile^2 u64), entry q of a slot being the tile's pixel at column q % tile, row q / tile.  Entries of a partial tile that
// fall outside the frame name no pixel and stay zero.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.h"
#include "pt_layout.h"

namespace pt {

constexpr uint32_t kNoPixel = 0xffffffffu;

// The tile pass's params: a frame's (npix = the compact accumulator's entries, open slots * tile^2; k_begin and the chunk fields
// are not used) and the list.
struct TileParams : FrameParams {
    const uint32_t *open;  // the open-tile list (device memory)
    uint32_t tile_shift;   // log2 of the tile edge
    uint32_t tiles_x;      // tiles per row of tiles
    uint32_t rows;         // image rows of the band
};

// framebuffer index of entry k of the compact accumulator, kNoPixel where the entry lies outside the frame
PT_HD uint32_t global_pixel(const TileParams &F, uint32_t k) {
    const uint32_t t = F.open[k >> (2u * F.tile_shift)];
    const uint32_t q = k & ((1u << (2u * F.tile_shift)) - 1u);
    const uint32_t ty = t / F.tiles_x, tx = t - ty * F.tiles_x;
    const uint32_t col = (tx << F.tile_shift) + (q & ((1u << F.tile_shift) - 1u));
    const uint32_t row = (ty << F.tile_shift) + (q >> F.tile_shift);
    if (col >= F.width || row >= F.rows) return kNoPixel;
    return F.idx_begin + row * F.width + col;
}

// one round of the tile pass: samples [s_begin, s_end) of every entry of the compact accumulator `acc`; the other arguments as
// launch_mega's (pt_kernels.h), total_rays[7] zeroed by the caller before every launch
void launch_tile_pass(hipStream_t st, uint32_t grid, const DevScene &S, const LdsLayout &L, const TileParams &F, unsigned long long *acc,
                      uint32_t s_begin, uint32_t s_end, uint32_t lane_spp, uint32_t n_split, unsigned long long *total_rays, char *stack_mem);

// The geometry of a call's tiles and its per-tile state (device memory, tiles entries each).
struct TileGrid {
    uint32_t width, rows;  // the band: whole rows
    uint32_t tile_shift, tiles_x, tiles;
    uint32_t *spp;            // samples every pixel of the tile holds
    uint32_t *na;             // ... and how many of them are in half A
    unsigned long long *err;  // E of the tile's last evaluation; kTileNoError (pt_device.h) before the first
};

// What a run of a step does with the compact accumulator once its samples are traced.  The tiles of a step are a CLASS: they
// all hold the same count and the same nA before it, and so after it.
struct TileLevel {
    const uint32_t *open;  // the list the run was traced with, n_open entries
    uint32_t n_open;
    const unsigned long long *acc;  // the compact accumulator: [3] planes of n_open * tile^2
    uint32_t to_a;       // the run's samples belong to half A: they are added to half A's sums too
    uint32_t evaluate;   // the step ends with this run: the tiles now hold `spp` samples, `na` of them in half A, and with
    uint32_t estimate;   // `estimate` get e(p), E and the decision (without it - a half is empty - they stay open and keep no E)
    uint32_t spp, na;
    float fa, fb, fn, w;         // (float) nA, nB, nA + nB and the weight of THE NOISE ESTIMATE (ptrace.h), host binary32
    unsigned long long q;        // floor(tile_error * 2^28): a tile closes iff E <= q * (its pixels)
    uint32_t *counters;          // [0] the tiles this step leaves open, [1] the tiles it closed; zeroed by the caller
};
// held / half_a: [3] planes of width * rows u64 in the call's pixel order.
void launch_tile_level(hipStream_t st, const TileGrid &G, const TileLevel &V, unsigned long long *held, unsigned long long *half_a);

// The re-decision and the class selection, one thread per tile.  Under q a tile is closed iff it has an E and E <= q * (its
// pixels inside the band); every other tile is open.  out[0] += the open tiles, out[1] += those of them that hold `cap` samples
// or more (they take none), out[2] += the closed tiles.  With a list, every open tile that holds `c` samples, `na` of them in
// half A, is appended to it through one integer atomic on *list_len (the order of a list does not matter: a slot only names
// where a tile's entries of the compact accumulator lie).  out, list_len: zeroed by the caller.
struct TileSelect {
    unsigned long long q;
    uint32_t cap, c, na;
    uint32_t *list, *list_len;  // NULL: count only
    uint32_t *out;
};
void launch_tile_select(hipStream_t st, const TileGrid &G, const TileSelect &S);

// Every pixel resolved over its tile's count (count 0: black), the counts (spp: may be NULL), e(p) of every pixel from the held
// sums and half A's at its tile's count and nA - the estimate of the tile's last evaluation, a step ending with one - or +inf
// where the tile has no E (error: width * rows floats, may be NULL), and *err_sum += E of every tile that has one (err_sum: may
// be NULL).
void launch_tile_resolve(hipStream_t st, const TileGrid &G, const unsigned long long *held, const unsigned long long *half_a,
                         float *out_rgb, uint32_t *spp, float *error, unsigned long long *err_sum);

}  // namespace pt
