// cudaraytracing_amd/csrc/crt_untile.h -- the index arithmetic and the kernel of the de-interleave that ends a multi-device frame
// (contract: include/crt.h, crt_multi_render_buffers; host code: crt_multi.hip): the gathered blocks of all ranks -> row-major planes.
//   layout   Rank r of `world` owns the 8x8 pixel tiles t with t % world == r and stores its k-th one (t = k * world + r) at pixel slots
//            [64 k, 64 k + 64) of every plane of its block, row by row inside the tile; slots of pixels beyond a ragged right / bottom
//            edge are padding.  A block is `stride` bytes: the wanted planes one after the other, each from a 16-byte boundary
//            (UntilePlane::src_off), a plane = slots x per_pixel elements of `elem` bytes.
//   kernel   One launch moves every plane of the table, which travels in the kernel's arguments.  One lane moves ONE element: a 4-byte
//            word of a word plane (f32 / i32, 1 or 3 words per pixel) or a byte of RGB8.  A workgroup is 256 consecutive elements of one
//            output row of one plane, so a wave's stores are 64 consecutive words (256 B) or bytes of the row: fully coalesced.  A tile
//            row is 8 pixels, contiguous in the block as in the frame, so its loads come in runs of 8 x per_pixel consecutive elements
//            (96 B for a 3-float plane).  Nothing wider than a word is taken: a row starts on a 16-byte boundary only if
//            width x per_pixel is a multiple of 4, a tile row's 8 x per_pixel words start at a multiple of 32 x per_pixel bytes in the
//            block but at 4 x per_pixel x (8 tx + j width) in the frame -- no width-independent alignment above 4 bytes exists on the
//            store side, and a word plane's source and destination are 4-byte aligned by construction (16-byte plane offsets, strides
//            and allocations).  Only pixels inside the frame are visited: no padding slot is read, nothing beyond a plane is written.
//            The launch is one-dimensional (block -> plane, row, chunk of the row) with the same number of chunks per row for every
//            plane -- that of a 3-element plane; the surplus workgroups of a 1-element plane leave at once.
// Like crt_pyramid.h this file includes nothing, so that tools/untile_host_check.cpp can compile this very text for the host behind
// tools/host_device.h.
#ifndef CRT_UNTILE_H
#define CRT_UNTILE_H

namespace crtk {

const uint32_t kUntileMaxPlanes = 13; // one per CRT_MULTI_* bit
const uint32_t kUntileBlock = 256;    // lanes per workgroup = elements of an output row per workgroup

struct UntilePlane {
    uint64_t src_off;   // byte offset of the plane in a rank's block (a multiple of 16)
    uint8_t* dst;       // row-major plane: width x height x per_pixel elements
    uint32_t per_pixel; // elements per pixel: 1 or 3
    uint32_t elem;      // bytes per element: 4 (f32 / i32) or 1 (RGB8)
};

struct UntileParams {
    const uint8_t* gathered; // world blocks of `stride` bytes
    uint64_t stride;
    uint32_t world, width, height, tiles_x;
    uint32_t chunks;         // workgroups per output row: untile_chunks(width)
    uint32_t n_planes;
    UntilePlane plane[kUntileMaxPlanes];
};

__host__ __device__ __forceinline__ uint64_t untile_align16(const uint64_t bytes) { return (bytes + 15u) & ~(uint64_t)15u; }
// the bytes of one plane in a rank's block, padded to the boundary the next one starts on
__host__ __device__ __forceinline__ uint64_t untile_plane_bytes(const uint64_t slots, const uint32_t per_pixel, const uint32_t elem)
{
    return untile_align16(slots * per_pixel * elem);
}
__host__ __device__ __forceinline__ uint32_t untile_tiles_x(const uint32_t width) { return (width + 7u) / 8u; }
__host__ __device__ __forceinline__ uint32_t untile_chunks(const uint32_t width) { return (uint32_t)(((uint64_t)width * 3u + kUntileBlock - 1u) / kUntileBlock); }
__host__ __device__ __forceinline__ uint64_t untile_grid(const UntileParams& P) { return (uint64_t)P.n_planes * P.height * P.chunks; }

// the tile of pixel (i, j)
__host__ __device__ __forceinline__ uint32_t untile_tile(const uint32_t i, const uint32_t j, const uint32_t tiles_x) { return (j >> 3) * tiles_x + (i >> 3); }
// the rank that owns a tile, and which of that rank's tiles it is
__host__ __device__ __forceinline__ uint32_t untile_rank(const uint32_t tile, const uint32_t world) { return tile % world; }
__host__ __device__ __forceinline__ uint32_t untile_local(const uint32_t tile, const uint32_t world) { return tile / world; }
// the pixel slot of (i, j) in its rank's planes
__host__ __device__ __forceinline__ uint64_t untile_slot(const uint32_t local, const uint32_t i, const uint32_t j)
{
    return (uint64_t)local * 64u + (j & 7u) * 8u + (i & 7u);
}
// the byte of element `comp` of pixel slot `slot` of a plane in the gathered blocks
__host__ __device__ __forceinline__ uint64_t untile_src_byte(const uint64_t stride, const uint32_t rank, const UntilePlane& pl, const uint64_t slot, const uint32_t comp)
{
    return (uint64_t)rank * stride + pl.src_off + (slot * pl.per_pixel + comp) * pl.elem;
}
// the byte of element `comp` of pixel (i, j) in the row-major plane
__host__ __device__ __forceinline__ uint64_t untile_dst_byte(const uint32_t width, const UntilePlane& pl, const uint32_t i, const uint32_t j, const uint32_t comp)
{
    return (((uint64_t)j * width + i) * pl.per_pixel + comp) * pl.elem;
}

// element e of output row j of plane pl: e = i * per_pixel + comp, inside the row
__device__ __forceinline__ void untile_element(const UntileParams& P, const UntilePlane& pl, const uint32_t j, const uint32_t e)
{
    const uint32_t i = pl.per_pixel == 3u ? e / 3u : e / pl.per_pixel;
    const uint32_t comp = e - i * pl.per_pixel;
    const uint32_t tile = untile_tile(i, j, P.tiles_x);
    const uint64_t slot = untile_slot(untile_local(tile, P.world), i, j);
    const uint8_t* src = P.gathered + untile_src_byte(P.stride, untile_rank(tile, P.world), pl, slot, comp);
    uint8_t* dst = pl.dst + untile_dst_byte(P.width, pl, i, j, comp);
    if (pl.elem == 4u) *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
    else *dst = *src;
}

// grid: untile_grid(P) workgroups of kUntileBlock lanes
__global__ __launch_bounds__(256) void k_untile_planes(const UntileParams P)
{
    const uint32_t b = blockIdx.x;
    const uint32_t rows = b / P.chunks, c = b - rows * P.chunks;
    const uint32_t p = rows / P.height, j = rows - p * P.height;
    const UntilePlane& pl = P.plane[p];
    const uint32_t e = c * kUntileBlock + threadIdx.x;
    if (e >= P.width * pl.per_pixel) return;
    untile_element(P, pl, j, e);
}

} // namespace crtk
#endif
