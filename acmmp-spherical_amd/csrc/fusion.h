// fusion.h -- device-side types and launchers of the depth-map fusion and the voxel-grid reduction
// (fusion.cpp drives them, fusion_kernels.hip implements them).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

namespace acmmp {

// One view of the fusion set (device pointers): depth (W x H), normals (3 floats per pixel, world
// frame as normals.dmb holds them), colour as the reference's float RGBA texture (4 per pixel, /255).
// used: one byte per pixel, 1 = the depth sample already contributed to a point of an earlier reference
// view of a duplicate-free scene pass (acmmp_fusion_run_scene with ACMMP_FUSE_UNIQUE); other passes ignore it.
struct FuseView {
    const float* depth;
    const float* normal;
    const float* rgba;
    int W, H;
    uint8_t* used;
};

// SimpleFusionKernel (ACMMP.cu:1662-1814) for reference view `ref` + compaction in pixel order:
// out_dense/flags are P-sized scratch, block_counts ceil(P/256) ints.
hipError_t launch_fuse(int model, const DevCam* cams, const FuseView* views, int ref, int W, int H, const int* srcs,
                       int n_src, float* out_dense, int* flags, int* block_counts, hipStream_t s);
// block_counts: valid pixels per 256-pixel chunk (written by launch_fuse); block_offsets: their prefix.
hipError_t launch_fuse_compact(int W, int H, const float* out_dense, const int* flags, const int* block_offsets,
                               float* out, hipStream_t s);
// One reference view of a whole-scene pass, all in stream order with no host step: SimpleFusionKernel with
// the per-pixel consistent-source mask (unique: depths read through the views' used masks), the chunk
// counts, their exclusive scan into block_offsets, *view_count = the view's points, *view_base = *running,
// *running += *view_count, and (unique) the marking of every contributing sample.  src_mask is P-sized scratch.
hipError_t launch_fuse_scene(int model, bool unique, const DevCam* cams, const FuseView* views, int ref, int W, int H,
                             const int* srcs, int n_src, float* out_dense, int* flags, uint32_t* src_mask,
                             int* block_counts, int* block_offsets, int* view_count, unsigned long long* running,
                             unsigned long long* view_base, hipStream_t s);
// Points and provenance of that view to the scene buffers at *view_base; nothing is written at or past `cap` points.
hipError_t launch_fuse_scatter_scene(int W, int H, const float* out_dense, const int* flags, const uint32_t* src_mask,
                                     const int* block_offsets, const unsigned long long* view_base, int ref_pos,
                                     unsigned long long cap, float* out, int* out_ref, int* out_pix, uint32_t* out_mask,
                                     hipStream_t s);

// Ordered compaction of one segment of a stage's items (points, voxels, entries, pairs, samples), in stream order with
// no host step.  A mark kernel writes flags[i] = item i0 + i is kept and counts[chunk] per 256 items; k_fuse_scan turns
// the counts into offsets and sets *seg_count = the segment's kept items, *seg_base = *running, *running += *seg_count;
// a scatter kernel gives kept item i the output position *seg_base + offsets[chunk] + its rank in the chunk and writes
// it there.  Nothing is written at or past `cap` outputs.  A pass zeroes *running, runs its segments (n <= 2^30 each:
// the offsets are 32-bit) in ascending order and ends with *running = the kept items of the whole pass.
struct Compaction {
    int* flags;                        // per item of a segment
    int* counts;                       // per 256-item chunk of a segment
    int* offsets;
    int* seg_count;
    unsigned long long* running;
    unsigned long long* seg_base;
    unsigned long long cap;
};

// Voxel-grid reduction of a scene cloud (acmmp_fusion_voxelize, include/acmmp.h).  Every launcher
// covers points [i0, i0 + n) of `pts` (9 floats each, n <= 2^30: one segment), one lane per point.
struct VoxGrid {
    float ox, oy, oz;          // origin
    float inv;                 // 1.0f / size, computed on the host
    float size;
};
// The hash table: open addressing with linear probing over `slots` = 2^log2_slots cells.  keys (~0 = empty),
// first (smallest scene index) and oid (output id of a kept voxel, ~0 = none) start as all-ones bytes, cnt as 0.
struct VoxTable {
    unsigned long long* keys;
    unsigned long long* first;
    unsigned long long* oid;
    uint32_t* cnt;
    unsigned long long slots;
    int log2_slots;
};
// Device words of a voxel run (all zero before it).
enum { kVoxErr = 0, kVoxRejected = 1, kVoxOccupied = 2, kVoxKept = 3, kVoxWrapped = 4, kVoxMaxProbe = 5, kVoxWords = 8 };
// mn[3] (pre-set to all-ones) := min over the points that pass the finiteness / magnitude test of ordered(x), (y), (z),
// ordered(f) being the order-preserving map of float bits to unsigned (vox_decode_ordered inverts it).
hipError_t launch_voxel_min(const float* pts, unsigned long long i0, int n, uint32_t* mn, hipStream_t s);
inline float vox_decode_ordered(uint32_t u) {
    const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}
// Insert pass: key, slot (CAS on keys), cnt += 1, first = min(first, index); st[kVoxRejected] += rejected points,
// st[kVoxErr] |= 1 when a probe sequence walked the whole table.
hipError_t launch_voxel_insert(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t,
                               unsigned long long* st, hipStream_t s);
// Over the slots: st[kVoxOccupied], st[kVoxKept] (cnt >= min_points), st[kVoxWrapped] (stored below the home slot),
// st[kVoxMaxProbe] (largest distance from the home slot + 1).
hipError_t launch_voxel_stats(VoxTable t, int min_points, unsigned long long* st, hipStream_t s);
// One segment, see Compaction: the points that are the first of a kept voxel; per kept point oid[slot] = its position
// and vslot[that id] = slot.  st[kVoxErr] |= 2 (mark) or 4 (scatter) for a failed lookup.
hipError_t launch_voxel_compact(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t, int min_points,
                                Compaction c, unsigned long long* vslot, unsigned long long* st, hipStream_t s);
// sums[9 * oid + k] += the point's quantised channel k (64-bit integer adds), for points of kept voxels.
hipError_t launch_voxel_accumulate(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t,
                                   unsigned long long* sums, unsigned long long* st, hipStream_t s);
// out[9 * v ..] and out_cnt[v] of voxels [0, nv) from their sums, in float64 rounded once to float32.
hipError_t launch_voxel_finalise(unsigned long long nv, const unsigned long long* vslot, VoxTable t,
                                 const unsigned long long* sums, VoxGrid g, float* out, int32_t* out_cnt, hipStream_t s);

// Cleaning the voxel cloud (acmmp_fusion_voxel_clean, include/acmmp.h): over the voxels [0, nv) of a
// voxel result, vslot[v] their slots in the table `t` that voxelize filled, one lane per voxel.
// Device words of a clean run (all zero before it; kCleanChanged is zeroed before every round).
enum { kCleanErr = 0, kCleanChanged = 1, kCleanUnsupported = 2, kCleanComps = 3, kCleanCompsKept = 4, kCleanKept = 5,
       kCleanWords = 6 };
// Per-voxel scratch of the component table, meaningful at a component's root (its smallest voxel): voxels, points
// (both zero before the run), dense id; and the two thresholds of step 5.
struct CleanComp {
    unsigned long long* voxels;
    unsigned long long* points;
    unsigned long long* id;
    unsigned long long min_voxels, min_points;
};
// nbmask[v] = bit (dz+1)*9 + (dy+1)*3 + (dx+1) per neighbouring voxel under `connectivity` (6, 18, 26); lab[v] = v when
// their number is >= min_neighbours, else ~0; words[kCleanUnsupported] += the others.  words[kCleanErr] |= 1 for a
// slot outside the table, 2 for a probe sequence that covered every slot.
hipError_t launch_clean_support(unsigned long long nv, const unsigned long long* vslot, VoxTable t, int connectivity,
                                int min_neighbours, uint32_t* nbmask, unsigned long long* lab, unsigned long long* words,
                                hipStream_t s);
// One labelling round (k_clean_round): words[kCleanChanged] |= 1 when a label was lowered; words[kCleanErr] |= 4 for
// a neighbour of nbmask that the table no longer gives, 8 for a label chain longer than nv.
hipError_t launch_clean_round(unsigned long long nv, const unsigned long long* vslot, VoxTable t, const uint32_t* nbmask,
                              unsigned long long* lab, unsigned long long* words, hipStream_t s);
// After the last round: c.voxels / c.points at every root, then words[kCleanComps], [kCleanCompsKept], [kCleanKept].
hipError_t launch_clean_sizes(unsigned long long nv, const unsigned long long* lab, const int32_t* cnt, CleanComp c,
                              unsigned long long* words, hipStream_t s);
// Voxels [i0, i0 + n), one segment, see Compaction: the roots to the component table and c.id[root]; then, once every
// segment's roots are through, the kept voxels to the clean cloud (out_vox: their voxel index).
hipError_t launch_clean_compact_roots(unsigned long long nv, unsigned long long i0, int n, const unsigned long long* lab,
                                      CleanComp c, Compaction k, long long* out_root, long long* out_voxels,
                                      long long* out_points, hipStream_t s);
hipError_t launch_clean_compact_kept(unsigned long long nv, unsigned long long i0, int n, const unsigned long long* lab,
                                     CleanComp c, Compaction k, const float* v_pts, const int32_t* v_cnt, float* out,
                                     int32_t* out_cnt,
                                     long long* out_comp, unsigned long long* out_vox, hipStream_t s);

// Visibility check of the voxel or clean cloud (acmmp_fusion_voxel_visibility, include/acmmp.h): over
// the entries [0, n) of `pts` (9 floats each), one lane per entry.
// List positions per workgroup row of the tally kernel: a list of more takes several rows and integer atomics.
constexpr int kVisChunk = 32;
// Device words of a visibility run (all zero before it).
enum { kVisSupport = 0, kVisConflict = 1, kVisOccluded = 2, kVisUnobserved = 3, kVisKept = 4, kVisNoSupport = 5,
       kVisConflicting = 6, kVisWords = 7 };
// tallies[3 e ..] = (support, conflict, occluded) of entry e over the views list[0 .. n_list) (indices into cams /
// views, every one set), the entry classed per view by its projection against the view's raw depth in the window
// of `radius` pixels.  More than kVisChunk positions: the tallies are zeroed and added to, else stored.
hipError_t launch_vis_tally(int model, const DevCam* cams, const FuseView* views, const int* list, int n_list,
                            const float* pts, unsigned long long n, float rel_tol, int radius, int32_t* tallies,
                            hipStream_t s);
// words[kVisSupport .. kVisUnobserved] += the class sums (unobserved = n_list - the three tallies), words[kVisKept],
// [kVisNoSupport], [kVisConflicting] += the entries with support >= min_support and conflict <= max_conflicts, those
// failing the first, those failing the second.
hipError_t launch_vis_count(unsigned long long n, const int32_t* tallies, int n_list, int min_support, int max_conflicts,
                            unsigned long long* words, hipStream_t s);
// Entries [i0, i0 + n), one segment, see Compaction: the kept entries' floats, counts and tallies in ascending order,
// and out_vox = their voxel index (src_vox[e], or e itself when src_vox is NULL).
hipError_t launch_vis_compact(unsigned long long i0, int n, const int32_t* tallies, int min_support, int max_conflicts,
                              Compaction c, const float* src_pts, const int32_t* src_cnt, float* out, int32_t* out_cnt,
                              int32_t* out_tal, const unsigned long long* src_vox, unsigned long long* out_vox,
                              hipStream_t s);

// Surface mesh of the voxel, clean or visible result (acmmp_fusion_voxel_mesh, include/acmmp.h).
// The sample table: open addressing as VoxTable.  keys (~0 = empty), rank (smallest e * 27 + offset index), ent (the
// entry whose own cell this is, ~0 = none) and sid (the sample's number) start as all-ones bytes.
struct MeshTable {
    unsigned long long* keys;
    unsigned long long* rank;
    unsigned long long* ent;
    unsigned long long* sid;
    unsigned long long slots;
    int log2_slots;
};
// Device words of a mesh run (all zero before it).
enum { kMeshErr = 0, kMeshOccupied = 1, kMeshWrapped = 2, kMeshMaxProbe = 3, kMeshValid = 4, kMeshCubes = 5, kMeshActive = 6,
       kMeshPairs = 7, kMeshUncoloured = 8, kMeshWords = 9 };
// Bits of a sample's flag byte (launch_mesh_cubes).
enum { kMeshCubeExists = 1, kMeshCubeActive = 2, kMeshSampleValid = 4, kMeshSampleInside = 8 };
// The per-sample arrays of a mesh result: packed cell, (S, n), remembered entry (-1 = none).
struct MeshSamples {
    unsigned long long* key;
    int32_t* tsdf;
    long long* ent;
    unsigned long long n;
};
// ekey[e] = the packed cell of entry e: t.keys[vslot[vox ? vox[e] : e]]; words[kMeshErr] |= 1 for an index outside.
hipError_t launch_mesh_keys(unsigned long long ne, const unsigned long long* vox, unsigned long long nv,
                            const unsigned long long* vslot, VoxTable t, unsigned long long* ekey,
                            unsigned long long* words, hipStream_t s);
// Pairs [p0, p0 + n) of the 27 ne (entry, offset) pairs, one lane each: the cell's slot (CAS on keys), rank =
// min(rank, p), ent = e for the entry's own cell; words[kMeshErr] |= 2 when a probe sequence walked the whole table.
hipError_t launch_mesh_insert(unsigned long long p0, int n, const unsigned long long* ekey, MeshTable m,
                              unsigned long long* words, hipStream_t s);
// Over the slots: words[kMeshOccupied], [kMeshWrapped], [kMeshMaxProbe] as launch_voxel_stats.
hipError_t launch_mesh_stats(MeshTable m, unsigned long long* words, hipStream_t s);
// Pairs [p0, p0 + n), one segment, see Compaction (c.cap = out.n): the pairs that own their cell's rank, in ascending
// order, number the samples: sid[slot], out.key, out.ent.
hipError_t launch_mesh_number(unsigned long long p0, int n, const unsigned long long* ekey, MeshTable m, Compaction c,
                              MeshSamples out, unsigned long long* words, hipStream_t s);
// out.tsdf[2 s ..] = (S, n) of every sample over the views list[0 .. n_list), as launch_vis_tally.
hipError_t launch_mesh_tsdf(int model, const DevCam* cams, const FuseView* views, const int* list, int n_list,
                            MeshSamples smp, VoxGrid g, float trunc, hipStream_t s);
// cflag[s] = the sample's kMesh* bits, then fbits[s] = bit a set when the pair (s, axis a) emits faces; words[kMeshValid],
// [kMeshCubes], [kMeshActive], [kMeshPairs] += their numbers, words[kMeshErr] |= 4 for a failed lookup.
hipError_t launch_mesh_cubes(MeshSamples smp, MeshTable m, int min_weight, uint8_t* cflag, uint8_t* fbits,
                             unsigned long long* words, hipStream_t s);
// Samples [i0, i0 + n), one segment, see Compaction: the active cubes' vertices (9 floats each) in ascending s, vid[s] =
// their number (all-ones before); src_pts: the entries' 9 floats.
hipError_t launch_mesh_vertices(unsigned long long i0, int n, MeshSamples smp, MeshTable m, VoxGrid g, const uint8_t* cflag,
                                const float* src_pts, Compaction c, float* verts, int32_t* vid, unsigned long long* words,
                                hipStream_t s);
// The (sample, axis) pairs [p0, p0 + n) of 3 ns, one segment, see Compaction: two triangles (6 indices) per flagged
// pair, in ascending order.
hipError_t launch_mesh_faces(unsigned long long p0, int n, MeshSamples smp, MeshTable m, const uint8_t* cflag,
                             const uint8_t* fbits, const int32_t* vid, Compaction c, int32_t* faces,
                             unsigned long long* words, hipStream_t s);

// The mesh result rendered into one camera (acmmp_fusion_mesh_render, include/acmmp.h).
// Device words of a render (all zero before it): kRenderLarge is also the queue's counter, kRenderCounts the first of
// the seven counts of step 8.
enum { kRenderSkipped = 0, kRenderSmall = 1, kRenderLarge = 2, kRenderCandidates = 3, kRenderCounts = 4, kRenderWords = 11 };
constexpr size_t kRenderItemBytes = 20;      // a queue entry: the face and its bound
constexpr int kRenderSmallMax = 256;         // candidates up to which a face is rendered by its own lane
// In stream order: k_render_setup over the nf faces (the skip test, the bound, the small faces' pixels, the others to
// `queue`, nf entries), k_render_large over the queue, k_render_resolve over the W x H pixels of `cam`.  keys: one word
// per pixel, all-ones bytes before the call.  raw: the view's raw depth map, or NULL for no agreement counts.
hipError_t launch_render(int model, const DevCam& cam, const float* verts, unsigned long long nv, const int32_t* faces,
                         unsigned nf, long long small_max, unsigned long long* keys, void* queue, const float* raw,
                         float rel_tol, float* depth, int32_t* face, float* normal, float* colour, unsigned long long* words,
                         hipStream_t s);

// Nearest-neighbour distances between two clouds (acmmp_fusion_cloud_distance, include/acmmp.h).
// A cloud for the device: point i is p[stride * i .. + 3), n points.  With xf set every point is read through the
// row-major 3x4 transform M (acmmp_fusion_set_cloud_transform, include/acmmp.h); with xf 0 M is not looked at.
// cls, where not NULL, holds the class byte of every point (launch_region_classify): a point whose class is not 0 reads
// as invalid, exactly as one with a coordinate that is not finite does.  NULL is the path without a region.
struct DistCloud {
    const float* p;
    int stride;
    unsigned long long n;
    int xf;
    double M[12];
    const uint8_t* cls;
};
// A uniform grid in float64: a coordinate's cell on axis a is floor(((double)x - o[a]) * inv), clamped to [0, cmax[a]].
// The host computes inv = 1.0 / cell and cmax from the targets' bounding box with the same two operations.
struct DistGrid {
    double o[3];
    double inv, cell;
    int cmax[3];
};
// The cell table: open addressing as VoxTable over keys (~0 = empty, all-ones bytes before the insert pass).  cnt is 0
// before the insert pass and holds a cell's list length after it; launch_dist_lists turns it into the cell's cursor,
// which ends at the list's end, and fills start.  A coarse table has keys only (start and cnt NULL).
struct DistTable {
    unsigned long long* keys;
    uint32_t* start;
    uint32_t* cnt;
    unsigned long long slots;
    int log2_slots;
};
// Device words of a distance call (all zero before it), then the summary of acmmp.h from kDistSummary on.  kDistMin holds
// six 32-bit words, all-ones before the call: the ordered minimum of x, y, z and the ordered minimum of -x, -y, -z over the
// valid targets (vox_decode_ordered; the second three negated give the maximum).
enum { kDistErr = 0, kDistValidTargets = 1, kDistOccupied = 2, kDistMaxList = 3, kDistRings = 4, kDistCursor = 5,
       kDistMin = 6, kDistSummary = 9, kDistWords = 9 + 268 };
// words[kDistMin ..] and words[kDistValidTargets] over the targets.
hipError_t launch_dist_bounds(DistCloud t, unsigned long long* words, hipStream_t s);
// Insert pass over the valid targets: the fine cell's slot in `fine` with cnt += 1, the coarse cell's slot in `coarse`;
// words[kDistErr] |= 1 when a probe sequence walked a whole table.
hipError_t launch_dist_insert(DistCloud t, DistGrid g, DistTable fine, DistGrid cg, DistTable coarse,
                              unsigned long long* words, hipStream_t s);
// Every occupied slot takes its list's start from words[kDistCursor] (the order of the slots is invisible), then every
// valid target j goes to its cell's list: list[pos] = (x, y, z, bits of j).  words[kDistOccupied], [kDistMaxList];
// words[kDistErr] |= 2 for a failed lookup.
hipError_t launch_dist_lists(DistCloud t, DistGrid g, DistTable fine, float4* list, unsigned long long* words,
                             hipStream_t s);
// The parameters of the query pass that are plain numbers.
struct DistQuery {
    float m2;                  // max_dist * max_dist in float32
    double k;                  // 1048576.0 / (double)max_dist
    int n_tau;
    float tau2[8];             // tau[i] * tau[i] in float32
    double lo[3], hi[3];       // the valid targets' bounding box
    int have_targets;          // 0: every query is unmatched and no table is read
};
// One lane per query: d2[i], nearest[i] and the summary at words[kDistSummary ..] (n_query is the host's);
// words[kDistRings] = the largest ring searched.
hipError_t launch_dist_query(DistCloud q, DistGrid g, DistTable fine, DistGrid cg, DistTable coarse, const float4* list,
                             DistQuery p, float* d2, int32_t* nearest, unsigned long long* words, hipStream_t s);
// One iteration of acmmp_fusion_cloud_align over the grid of a distance call's build: the queries are the points
// 0, stride, 2 stride, ... of q (read through q's transform), t is the target cloud the grid was built from.  rec: the
// ACMMP_ALIGN_RECORD_WORDS words of the record, zero before the launch (n_query is the host's); words: the distance
// call's words, of which [kDistErr] (|= 8: a winner that is no valid target) and [kDistRings] are written.
constexpr int kAlignWords = ACMMP_ALIGN_RECORD_WORDS;
hipError_t launch_align_iter(DistCloud q, unsigned long long stride, DistCloud t, DistGrid g, DistTable fine, DistGrid cg,
                             DistTable coarse, const float4* list, DistQuery p, double kq, unsigned long long* words,
                             unsigned long long* rec, hipStream_t s);
// One iteration of acmmp_fusion_cloud_align_plane: as launch_align_iter, with the normal of data point i at q.p[q.stride
// * i + 3 .. + 6) (q.stride >= 6) turned by q's transform, and the pivot g of the levers.  rec: the
// ACMMP_ALIGN_PLANE_RECORD_WORDS words, zero before the launch (n_query and the pivot are the host's).
constexpr int kAlignPlaneWords = ACMMP_ALIGN_PLANE_RECORD_WORDS;
struct AlignPivot { long long g[3]; };
hipError_t launch_align_plane_iter(DistCloud q, unsigned long long stride, DistCloud t, DistGrid g, DistTable fine,
                                   DistGrid cg, DistTable coarse, const float4* list, DistQuery p, double kq,
                                   AlignPivot pivot, unsigned long long* words, unsigned long long* rec, hipStream_t s);

// Point-to-triangle distances from a cloud to the mesh result (acmmp_fusion_surface_distance, include/acmmp.h;
// DESIGN.md §8).  The mesh for the device: face j is the vertices faces[3 j .. + 3) of v, read as dist_load reads a point.
struct SurfMesh {
    DistCloud v;
    const int32_t* faces;
    unsigned nf;
};
// Device words of a surface call: a distance call's (kDistValidTargets counts the valid faces, kDistCursor the
// registrations listed), then the plan and the overflow list's cursor.
enum { kSurfSmall = kDistWords, kSurfLarge, kSurfRegs, kSurfLargeCursor, kSurfWords };
constexpr int kSurfSmallMax = 64;            // cells up to which a face is registered in the grid
constexpr size_t kSurfEntryWords = 3;        // a list entry in float4s: (A, bits of j), (B, 0), (C, 0) -- 48 bytes
// words[kDistMin ..] over the vertices of the valid faces and words[kDistValidTargets] = their number.
hipError_t launch_surf_bounds(SurfMesh m, unsigned long long* words, hipStream_t s);
// words[kSurfSmall], [kSurfLarge], [kSurfRegs]: the faces registered, the large faces (small_max < 0: every face) and
// the (face, cell) registrations of grid g.
hipError_t launch_surf_plan(SurfMesh m, DistGrid g, long long small_max, unsigned long long* words, hipStream_t s);
// The count pass, the cells' runs and the scatter: every small face into the list of every cell its box overlaps, every
// large face into `large` (cap_large entries).  list holds cap_list entries.  words[kDistErr] |= 1 a full table, |= 2 a
// failed lookup or a list overrun; words[kDistCursor] and [kSurfLargeCursor] end at the two lists' lengths.
hipError_t launch_surf_lists(SurfMesh m, DistGrid g, DistTable fine, long long small_max, float4* list,
                             unsigned long long cap_list, float4* large, unsigned long long cap_large,
                             unsigned long long* words, hipStream_t s);
// One lane per query, as launch_dist_query: the box reject, the n_large overflow entries, the rings.
hipError_t launch_surf_query(DistCloud q, DistGrid g, DistTable fine, const float4* list, const float4* large,
                             unsigned n_large, DistQuery p, float* d2, int32_t* nearest, unsigned long long* words,
                             hipStream_t s);

// Evaluation regions (acmmp_fusion_set_region, include/acmmp.h).  A region for the device: the planes by
// value, the polygon as n_vertices (u, v) pairs of doubles in device memory (0 = no prism), the grid's bits in device
// memory (dims[0] = 0: no grid).
struct RegionDev {
    int n_planes;
    double planes[4 * ACMMP_REGION_MAX_PLANES];
    int n_vertices, axis;
    double axis_min, axis_max;
    const double* poly;
    int dims[3];
    double o[3], cell;
    const uint8_t* bits;
};
// Device words of a classify pass (all zero before it): the counts of acmmp_fusion_region_classify, in its order.
enum { kRegionWords = ACMMP_REGION_COUNT_WORDS };
// One lane per point of c (read through c's stride and transform; c.cls is not looked at): cls[i] = the class byte of
// the definition, words[0 .. kRegionWords) += the counts, one atomic per word per workgroup.  words may be NULL (the
// pre-pass of a measuring call, which needs no counts).
hipError_t launch_region_classify(DistCloud c, RegionDev r, uint8_t* cls, unsigned long long* words, hipStream_t s);

// Area-uniform samples of the mesh result (acmmp_fusion_mesh_sample, include/acmmp.h).
// Device words of a sample call (all zero before it).
enum { kSampleTotal = 0, kSampleSkipped = 1, kSampleWords = 2 };
// Steps 1 to 4 in stream order, one lane per face, then one workgroup over the chunks of 256 faces: loc[f] = the samples
// of the faces before f in its chunk, chunk_tot[c] and base[c] = the samples of chunk c and of the chunks before it
// (ceil(nf / 256) of each), words[kSampleTotal] = N, words[kSampleSkipped] += the invalid faces.  s2 = spacing^2.
hipError_t launch_sample_count(const float* verts, unsigned long long nv, const int32_t* faces, unsigned nf, double s2,
                               unsigned long long seed, unsigned long long* loc, unsigned long long* chunk_tot,
                               unsigned long long* base, unsigned long long* words, hipStream_t s);
// Steps 5 and 6, one lane per sample: sample i < N (the host's copy of words[kSampleTotal]) to out[9 i ..] and out_face[i].
hipError_t launch_sample_emit(const float* verts, unsigned long long nv, const int32_t* faces, unsigned nf,
                              unsigned long long seed, const unsigned long long* loc, const unsigned long long* base,
                              unsigned long long N, float* out, int32_t* out_face, hipStream_t s);

}  // namespace acmmp
