// pt_kernels_tile.hip - the translation unit of pt_ctx_render_adaptive's tile pass: the same source as pt_kernels.hip, of which
// PT_TU_TILE leaves the megakernel's two bodies - compiled for TileParams (pt_tile.h), whose global_pixel reads the open-tile
// list, under the names k_tile_mega / k_tile_mega_cand - and launch_tile_pass.  A unit of its own so that the frame kernels'
// assembly (pt_kernels.s, pt_kernel_isa_hash()) is what it was; built with the options of pt_kernels.hip (Makefile: MLLVM).
#define PT_TU_TILE 1
#include "pt_kernels.hip"
