// tools/untile_host_check.cpp -- the de-interleave of a multi-device frame (cudaraytracing_amd/csrc/crt_untile.h: the index arithmetic
// and k_untile_planes, as they are) compiled for the HOST and run against a plain restatement, for AddressSanitizer / UBSan runs without
// a device.  tools/host_device.h stands in for the device; the kernel has no cross-lane operation, so a launch is a plain loop over
// blocks and threads.
// The blocks of all ranks are filled so that every source word says where it is -- rank, pixel slot, plane and component -- and every
// padding slot and every byte between planes holds a value no pixel may show.  Every destination plane is a vector of exactly its size
// plus guard bytes on both sides: a store beyond the guards is a sanitizer report, one into them a failed check.  Covered: widths and
// heights 1 .. 17 (ragged on either edge, one to nine tiles) with 1 .. 5 ranks (never more ranks than tiles), a few wider frames whose
// rows take several workgroups, every element size (RGB8; 1 and 3 words per pixel), and plane tables with gaps: blocks that hold planes
// the table does not name, and tables of a few planes only.
//
// tests/test_untile_host.py builds and runs it, plain and sanitised, as `program - out` (out: a digest of every destination byte):
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/untile_host_check.cpp -o /tmp/untile_host_check && /tmp/untile_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_device.h"

#include "crt_untile.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (g_fail < 50) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } g_fail++; } \
    } while (0)

// the planes of include/crt.h's CRT_MULTI_* bits, in their order: elements per pixel, bytes per element
static const uint32_t kKinds[kUntileMaxPlanes][2] = {{3, 1}, {3, 4}, {3, 4}, {3, 4}, {3, 4}, {3, 4}, {3, 4}, {1, 4}, {1, 4}, {1, 4}, {1, 4}, {3, 4}, {3, 4}};
static const uint32_t kGuard = 32;
static const uint8_t kGuardByte = 0xa5, kUnwritten = 0x5a, kPadding = 0xee;

// what the source holds at (rank, slot, plane, component): a word that says so (its top byte is 0x40: no padding word looks like it) ...
static uint32_t word_at(uint32_t rank, uint64_t slot, uint32_t plane, uint32_t comp)
{
    return 0x40000000u | (rank << 24 & 0x07000000u) | (plane << 20) | (comp << 18) | (uint32_t)slot;
}
// ... or, in a byte plane, a byte that mixes the four (never the padding byte)
static uint8_t byte_at(uint32_t rank, uint64_t slot, uint32_t plane, uint32_t comp)
{
    const uint8_t b = (uint8_t)(rank * 37u + (uint32_t)slot * 3u + plane * 11u + comp * 5u + 1u);
    return b == kPadding ? (uint8_t)0x11 : b;
}

static uint64_t g_digest = 1469598103934665603ull;
static void digest(const uint8_t* p, size_t n)
{
    for (size_t i = 0; i < n; i++) g_digest = (g_digest ^ p[i]) * 1099511628211ull;
}

// layout: the planes the blocks hold; table: the ones the kernel is asked to move (a subset of layout)
static void run_case(uint32_t w, uint32_t h, uint32_t world, uint32_t layout, uint32_t table)
{
    // ---- the contract, restated: interleaved 8x8 tiles, ceil(tiles / world) tiles of 64 slots per rank ----
    const uint32_t tx = (w + 7) / 8, ty = (h + 7) / 8, tiles = tx * ty;
    const uint64_t slots = (uint64_t)((tiles + world - 1) / world) * 64;
    uint64_t off[kUntileMaxPlanes], stride = 0;
    for (uint32_t p = 0; p < kUntileMaxPlanes; p++) {
        off[p] = stride;
        if (layout >> p & 1) stride += (slots * kKinds[p][0] * kKinds[p][1] + 15) / 16 * 16;
    }
    std::vector<uint8_t> gathered((size_t)(stride * world), kPadding); // exactly the blocks: a read beyond them is a report
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) {
            const uint32_t tile = (j / 8) * tx + i / 8, rank = tile % world, local = tile / world;
            const uint64_t slot = (uint64_t)local * 64 + (j % 8) * 8 + i % 8;
            for (uint32_t p = 0; p < kUntileMaxPlanes; p++) {
                if (!(layout >> p & 1)) continue;
                const uint32_t pp = kKinds[p][0], el = kKinds[p][1];
                for (uint32_t c = 0; c < pp; c++) {
                    uint8_t* s = gathered.data() + rank * stride + off[p] + (slot * pp + c) * el;
                    if (el == 4) { const uint32_t v = word_at(rank, slot, p, c); std::memcpy(s, &v, 4); }
                    else *s = byte_at(rank, slot, p, c);
                }
            }
        }

    // ---- the kernel's own text ----
    std::vector<std::vector<uint8_t>> dst(kUntileMaxPlanes);
    UntileParams U{};
    U.gathered = gathered.data(); U.stride = stride; U.world = world; U.width = w; U.height = h;
    U.tiles_x = untile_tiles_x(w); U.chunks = untile_chunks(w);
    for (uint32_t p = 0; p < kUntileMaxPlanes; p++) {
        const size_t n = (size_t)w * h * kKinds[p][0] * kKinds[p][1];
        dst[p].assign(n + 2 * kGuard, kGuardByte);
        std::fill(dst[p].begin() + kGuard, dst[p].end() - kGuard, kUnwritten);
        if (table >> p & 1) {
            CHECK(untile_plane_bytes(slots, kKinds[p][0], kKinds[p][1]) == (slots * kKinds[p][0] * kKinds[p][1] + 15) / 16 * 16, "plane bytes");
            U.plane[U.n_planes++] = UntilePlane{off[p], dst[p].data() + kGuard, kKinds[p][0], kKinds[p][1]};
        }
    }
    CHECK(U.tiles_x == tx, "tiles_x");
    hipLaunchKernelGGL(k_untile_planes, dim3((uint32_t)untile_grid(U)), dim3(kUntileBlock), 0, nullptr, U);

    // ---- every destination element, the guards, and the planes the table does not name ----
    for (uint32_t p = 0; p < kUntileMaxPlanes; p++) {
        const uint32_t pp = kKinds[p][0], el = kKinds[p][1];
        const std::vector<uint8_t>& d = dst[p];
        for (uint32_t g = 0; g < kGuard; g++)
            CHECK(d[g] == kGuardByte && d[d.size() - 1 - g] == kGuardByte, "%ux%u world %u: a guard byte of plane %u was written", w, h, world, p);
        if (!(table >> p & 1)) {
            for (size_t b = kGuard; b < d.size() - kGuard; b++) CHECK(d[b] == kUnwritten, "%ux%u world %u: plane %u is not in the table and was written", w, h, world, p);
            continue;
        }
        for (uint32_t j = 0; j < h; j++)
            for (uint32_t i = 0; i < w; i++) {
                const uint32_t tile = (j / 8) * tx + i / 8, rank = tile % world, local = tile / world;
                const uint64_t slot = (uint64_t)local * 64 + (j % 8) * 8 + i % 8;
                for (uint32_t c = 0; c < pp; c++) {
                    const uint8_t* at = d.data() + kGuard + (((size_t)j * w + i) * pp + c) * el;
                    if (el == 4) {
                        uint32_t got;
                        std::memcpy(&got, at, 4);
                        CHECK(got == word_at(rank, slot, p, c), "%ux%u world %u plane %u (%u, %u).%u: %08x, expected %08x", w, h, world, p, i, j, c, got, word_at(rank, slot, p, c));
                    } else CHECK(*at == byte_at(rank, slot, p, c), "%ux%u world %u plane %u (%u, %u).%u: %02x, expected %02x", w, h, world, p, i, j, c, *at, byte_at(rank, slot, p, c));
                }
            }
        digest(d.data(), d.size());
    }
}

int main(int argc, char** argv)
{
    const uint32_t all = (1u << kUntileMaxPlanes) - 1u;
    // blocks and tables: everything; a block of everything with a table of every other plane (gaps between the planes moved); blocks of
    // a few planes only (other offsets): the variance alone, depth and tri, RGB with the emission
    const uint32_t masks[5][2] = {{all, all}, {all, 0x0aaau}, {1u << 2, 1u << 2}, {1u << 7 | 1u << 9, 1u << 7 | 1u << 9}, {1u | 1u << 11, 1u | 1u << 11}};
    int cases = 0;
    auto shape = [&](uint32_t w, uint32_t h, uint32_t world) {
        for (const auto& m : masks) { run_case(w, h, world, m[0], m[1]); cases++; }
    };
    for (uint32_t w = 1; w <= 17; w++)
        for (uint32_t h = 1; h <= 17; h++)
            for (uint32_t world = 1; world <= 5; world++)
                if (world <= ((w + 7) / 8) * ((h + 7) / 8)) shape(w, h, world);
    // rows of more than one workgroup: 3 x 86 = 258 elements is the first; 100 and 200 are ragged, 256 is not
    const uint32_t wide[4][3] = {{86, 3, 2}, {100, 9, 3}, {200, 5, 4}, {256, 8, 5}};
    for (const auto& s : wide) shape(s[0], s[1], s[2]);
    std::printf("%d cases, %d failures\n", cases, g_fail);
    if (argc > 2) {
        FILE* f = std::fopen(argv[2], "wb");
        if (!f) { std::printf("cannot write %s\n", argv[2]); return 2; }
        std::fwrite(&g_digest, sizeof(g_digest), 1, f);
        std::fclose(f);
    }
    return g_fail ? 1 : 0;
}
