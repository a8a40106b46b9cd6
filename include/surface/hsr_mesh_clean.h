/*
 * hsr_mesh_clean.h — C ABI of the connected components of a triangle mesh and of the removal of some of them (libhsr_rast.so), DESIGN.md
 * §7 row 18: the step between "extract" (include/ext/hsr_tsdf.h) and "score" (include/eval/hsr_mesh_eval.h, include/recon/
 * hsr_mesh_depth.h) that drops floaters and stray shells (hsr_utils/mesh_clean.py).  In Open3D's words: cluster_connected_triangles,
 * remove_triangles_by_mask and remove_unreferenced_vertices.  The reference has no mesh and its family leaves the device here, so nothing
 * is pinned by reference outputs: the rules are RESTATED below, and tests/mesh_clean_ref.py restates them once more in numpy.  The header
 * lives under include/surface/: the prototypes under include/hsr_*.h and include/ext/ are counted sets (tests/test_abi.py), and
 * include/eval/, include/recon/ and include/sensor/ hold exactly one header each (the suites of those headers); these are bound under this
 * header's key in diff_gaussian_rasterization/_abi.py SURFACE_HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous.  Everything runs on `stream`; no entry point allocates or synchronises with the host.
 * Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in hsr_last_error() (hsr_rasterizer.h) that
 * starts "mesh_components: " or "mesh_select: ".  Integer work only: every output is a unique function of the inputs, two runs give the
 * same bytes, and nothing depends on how the device schedules the work.
 *
 * A face f of `faces` (int32 [F,3]) is VALID when its three indices lie in 0..V-1; a repeated index is allowed.  An invalid face
 * connects nothing, is counted nowhere and is never kept.
 *
 * hsr_mesh_components — two vertices are connected when a valid face names both; a component is a class of the closure of that relation.
 *   out_label      int32 [V]: the smallest vertex index of the component of v.  A vertex that no valid face names is its own component.
 *   out_face_count int32 [V]: at r = a label, the number of valid faces of that component (every vertex of a valid face has the same
 *                             label, so a face belongs to one component); 0 at every index that is not a label.
 *   V == 0 launches nothing.  F == 0 writes out_label[v] = v and zero counts.
 *   Refused: V < 0 or F < 0; a NULL faces with F > 0; a NULL out_label or out_face_count with V > 0.
 *
 *   How (csrc/hsr_mesh_clean.hip): out_label serves as the parent array of a lock-free union-find in which the larger root is always
 *   linked under the smaller one, so parent[x] <= x at all times and the root of a finished component is its smallest index; a lane per
 *   face unites (a, b) and (b, c) in ONE pass, with no "repeat until nothing changes" and no flag read by the host.  No lane waits for
 *   another: a retry follows only a compare-and-swap that another lane won, and continues from the value that compare-and-swap returned,
 *   so every step of a walk strictly descends.  THE BELT: every walk carries a step count and stops at a cap derived from V
 *   (2 * V + HSR_MESH_CLEAN_SLACK steps an edge, V + HSR_MESH_CLEAN_SLACK a vertex in the flatten) that cannot be reached while
 *   parent[x] <= x holds.  A lane that reaches it stores -1, a value no count takes, to out_face_count at the first vertex of its face
 *   (at its own vertex in the flatten) and stops; the counting launch never adds to a negative entry.  So:
 *     THE gave_up RULE: a walk gave up if and only if out_face_count has a negative entry; labels and counts are then not to be used.
 *   hsr_mesh_components takes no scratch and has no other output to say so; hsr_mesh_select has no walk and cannot give up, and its
 *   out_counts[2] is the word in which a caller carries (out_face_count < 0).sum() to the host in the one read it makes anyway
 *   (hsr_utils.mesh_clean.clean_mesh adds it on the device and raises when the word is not 0).
 *
 * hsr_mesh_select_scratch_bytes — a host function that launches nothing: the bytes hsr_mesh_select needs for V vertices and F faces: the
 * new index of every vertex (4 bytes each) and one count per block of HSR_MESH_CLEAN_BLOCK faces and of HSR_MESH_CLEAN_BLOCK vertices (4
 * bytes each), each array rounded up to 16 bytes, and 16 bytes more.  Monotone in V and in F, positive at V = F = 0; 0 for a negative
 * argument (no call with one is accepted).
 *
 * hsr_mesh_select — the faces of the components a caller keeps, and the vertices they use, both in their old order.
 *   label          int32 [V]: out_label of hsr_mesh_components (any int32 [V] is accepted: a face whose label[faces[f][0]] is outside
 *                             0..V-1 is dropped)
 *   keep_by_label  uint8 [V]: read at labels only
 *   A valid face f is KEPT when keep_by_label[label[faces[f][0]]] != 0; a vertex is kept when a kept face names it.  With F' kept faces
 *   and V' kept vertices:
 *   out_faces  int32 [F,3]: rows 0..F'-1 hold the kept faces in the order they had, in the new vertex numbering; rows from F' on are
 *                           not written
 *   out_source int32 [V]:   entries 0..V'-1 hold the old index of each new vertex, ascending (new vertex n is old vertex out_source[n]);
 *                           entries from V' on are not written
 *   out_counts int64 [3]:   {F', V', 0}: the third word is the gave_up word of the rule above, always 0 from this call
 *   Positions, colours and labels of the new vertices are attribute.index_select(0, out_source[:V']): one torch call each, no kernel.
 *   Refused: V < 0 or F < 0; a NULL faces or out_faces with F > 0; a NULL label, keep_by_label or out_source with V > 0; a NULL
 *   out_counts; a NULL scratch, one that is not 16-byte aligned, or scratch_bytes below hsr_mesh_select_scratch_bytes(V, F).
 *
 *   How: an order-preserving compaction in three phases — counts per block of HSR_MESH_CLEAN_BLOCK items, one workgroup that scans the
 *   counts of both lists and writes out_counts, and a scatter by each item's rank in its block (csrc/hsr_block.h).  No workgroup polls
 *   another.  The marks of the used vertices are zeroed on the stream inside the call, so a scratch carries nothing from one call to the
 *   next; many lanes may store the same mark.  V and F go up to 2^31-1; an index into [F,3] is 64-bit.
 */
#ifndef HSR_MESH_CLEAN_H_INCLUDED
#define HSR_MESH_CLEAN_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define HSR_MESH_CLEAN_BLOCK 256
#define HSR_MESH_CLEAN_SLACK 64

#ifdef __cplusplus
extern "C" {
#endif

int hsr_mesh_components(int V, int F, const int* faces, int* out_label, int* out_face_count, void* stream);

size_t hsr_mesh_select_scratch_bytes(int V, int F);

int hsr_mesh_select(int V, int F, const int* faces, const int* label, const uint8_t* keep_by_label, int* out_faces, int* out_source,
                    int64_t* out_counts, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MESH_CLEAN_H_INCLUDED */
