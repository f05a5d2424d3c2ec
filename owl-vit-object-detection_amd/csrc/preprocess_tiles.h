// What the tile resampler (preprocess.hip) and its colour path (color_jitter.hip) share: Pillow's fixed-point clip, the tile descriptor, the rows a thread takes.
#pragma once
#include "common.h"

#define PIL_PRECISION_BITS 22

__device__ __forceinline__ unsigned char pil_clip8(int v) {
    v >>= PIL_PRECISION_BITS;
    return (unsigned char)min(255, max(0, v));
}

// A TILE is one resample: source box -> a cw x ch rectangle ("cell") of output image b.  desc[i] = 18 int64 (device memory); the caller guarantees that the
// tiles of an output image cover it exactly (preprocess.py checks it on the host).
struct TileDesc { const unsigned char* src; long long H, W; const int* bx; const int* kx; long long ksx; const int* by; const int* ky; long long ksy;
                  long long y_first, n_rows, tmp_off, b, x0, y0, cw, ch, flip; };

// A thread produces TILE_ROWS vertically adjacent pixels: a quarter of the workgroups (most of a mosaic's grid lies outside the small cells and only leaves
// again), and in the horizontal pass one read of a column's weights serves four source rows.  Integer sums: the grouping cannot change a bit.
// (Tried: gridDim.x workgroups per tile walking the tile's 256 x TILE_ROWS units, so that no workgroup starts without work -- slower at g = 1 and 2, equal
// at g = 3, profiles/augment.md: the passes are bound by their byte loads per tap, not by the empty workgroups.)
#define TILE_ROWS 4

// preprocess.hip: the horizontal pass of a tile list (pp_tile_h_kernel), for the colour path's entry in color_jitter.hip
int pp_tile_h_launch(hipStream_t s, const TileDesc* desc, int64_t n_tiles, int64_t max_rows, unsigned char* tmp, int64_t out_w);
