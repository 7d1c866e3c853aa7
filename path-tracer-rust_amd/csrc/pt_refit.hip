// pt_refit.hip — pt_ctx_set_object's device side: the BVH of a translated mesh refit in place (pt_refit.h states the steps; the
// kernels only hand each lane its item).  A translation unit of its own, COMMON alone: the arithmetic is a stated contract whose
// divisions and square roots are the compiler's correctly rounded ones, and pt_kernels.s - pt_kernel_isa_hash() - stays the pass
// kernels'.  Memory: a lane reads its leaf's records (88 B each, strided by lane - a leaf's lines are touched once, by one lane)
// and gathers 36 B triangles by id; the tables of a 640 000-triangle mesh are 60 MB, read and written once per edit.  No lane
// waits for another: a height of the tree is a launch, and the stream orders the launches.
#include "pt_refit.h"

namespace pt {

namespace {

constexpr uint32_t kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void k_refit_leaves(RefitTables T, const RefitLeaf *__restrict__ leaves, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n) refit_leaf(T, leaves[i]);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_nodes(BvhNode *nodes, const RefitNode *__restrict__ items, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n) refit_node(nodes, items[i]);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_wide(BvhNode4 *nodes4, const BvhNode *__restrict__ nodes,
                                                            const RefitWide *__restrict__ items, uint32_t n) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n) refit_wide(nodes4, nodes, items[i]);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_materials(SurfRec *surf, uint32_t n, MatRec mm) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < n) surf_material(surf[i], mm, true);
}

uint32_t blocks_for(uint32_t n) { return (n + kRefitBlock - 1u) / kRefitBlock; }

}  // namespace

void launch_refit_leaves(hipStream_t st, const RefitTables &T, const RefitLeaf *leaves, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_refit_leaves, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, T, leaves, n);
}

void launch_refit_nodes(hipStream_t st, BvhNode *nodes, const RefitNode *items, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_refit_nodes, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, nodes, items, n);
}

void launch_refit_wide(hipStream_t st, BvhNode4 *nodes4, const BvhNode *nodes, const RefitWide *items, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_refit_wide, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, nodes4, nodes, items, n);
}

void launch_refit_materials(hipStream_t st, SurfRec *surf, uint32_t n, const MatRec &mm) {
    if (n) hipLaunchKernelGGL(k_refit_materials, dim3(blocks_for(n)), dim3(kRefitBlock), 0, st, surf, n, mm);
}

}  // namespace pt
