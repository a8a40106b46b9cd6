/*
 * hsr_mesh_depth.h — C ABI of the depth image of a triangle mesh from a given view (libhsr_rast.so), DESIGN.md §7 row 16: what "Depth
 * L1" of a run's mesh against a ground-truth mesh is computed from (hsr_utils/mesh_depth.py), and a depth image of a ground-truth mesh
 * from any pose for whoever wants one.  The reference has no mesh evaluation and its family leaves the device for Open3D here, so
 * nothing is pinned by reference outputs: the rule is RESTATED below, and tests/mesh_depth_ref.py restates it once more in numpy.  The
 * header lives under include/recon/: the prototypes under include/hsr_*.h and include/ext/ are counted sets (tests/test_abi.py) and
 * include/eval/ holds exactly one header (tests/test_mesh_eval_cpu.py); these are bound under this header's key in
 * diff_gaussian_rasterization/_abi.py RECON_HEADERS.
 *
 * All pointers are DEVICE pointers and contiguous, except `w2c`: a HOST array of 16 floats (row-major world-to-camera, rows 0..2 are
 * read) that is copied into the kernel arguments by value.  Everything runs on `stream`; no entry point allocates or synchronises with
 * the host.  Every refusal returns HSR_ERR_INVALID_ARGUMENT (-1) before any device work, with a message in hsr_last_error()
 * (hsr_rasterizer.h) that starts "mesh_depth: ".  The file is built without contraction: every float32 operation below is rounded
 * once, in exactly the stated order, and the numpy restatement matches bit for bit.
 *
 * hsr_mesh_depth_scratch_bytes — a host function that launches nothing: the bytes hsr_mesh_depth needs for an image of H x W and a
 * mesh of F faces: the key image (8 bytes a pixel), the list of large faces (4 bytes a face) and its counter, each rounded up to 16
 * bytes.  Monotone in F and in H * W, positive at F = 0; 0 for a negative argument (no call with one is accepted).
 *
 * hsr_mesh_depth — ONE view per call, as hsr_mesh_seen and hsr_tsdf_integrate: F faces int32 [F,3] over V vertices float32 [V,3],
 * seen through w2c and the pinhole (fx, fy, cx, cy) with pixel centres at integer coordinates, as everywhere in this project.
 *   out_depth float32 [H,W]: the depth along the camera's axis of the nearest face the ray of the pixel centre meets; 0 where none
 *   out_face  int32 [H,W]:   that face; -1 where none
 * THE RESULT IS DEFINED BY THE RULE BELOW AND NOTHING ELSE.
 *
 * The face.  Its camera-space corners A, B, C come from the chain of csrc/hsr_project.h (one device function, shared with
 * hsr_tsdf_integrate and hsr_mesh_seen):  xc = ((m00 * px + m01 * py) + m02 * pz) + m03, likewise yc and zc.  With
 *   cross(P, Q) = (Py * Qz - Pz * Qy,  Pz * Qx - Px * Qz,  Px * Qy - Py * Qx):
 *   nA = cross(B, C),  nB = cross(C, A),  nC = cross(A, B),  det = (Ax * nAx + Ay * nAy) + Az * nAz
 * A face takes NO part when one of its indices is outside 0..V-1, a camera-space coordinate is not finite, a component of the three
 * crosses is not finite, det is not finite, det is 0, or ALL THREE corners have zc < near.  The last clause is what makes a mesh that
 * surrounds the camera affordable: a point inside such a face has a depth below near, so the face could hit a pixel only by the rounding
 * of det / s, and without the clause every face behind the camera — half of a room seen from inside — would be tested at every pixel
 * of the image by the next rule.
 *
 * The box of a face, x0..x1 by y0..y1, the only pixels the face is tested at:
 *   a corner with zc < near (one or two of them: the face crosses z = near): the box is the whole image.  Otherwise, per corner,
 *   u = fx * (xc / zc) + cx,  v = fy * (yc / zc) + cy,  and
 *   x0 = floorf(min u) - 1,  x1 = ceilf(max u) + 1,  y0 = floorf(min v) - 1,  y1 = ceilf(max v) + 1                       (float32)
 *   the box is EMPTY when x1 < 0, x0 > W-1, y1 < 0 or y0 > H-1 (against (float)(W-1), (float)(H-1));  else each bound is clamped in
 *   float to the image, x0 = max(x0, 0), x1 = min(x1, W-1), likewise y, BEFORE the conversion to int: an infinite u never reaches (int).
 *   u and v are never NaN: the coordinates are finite, zc >= near > 0, and fx, fy, cx, cy are finite (refused otherwise).
 *
 * The hit test of face f at the pixel (x, y) of its box:
 *   rx = ((float)x - cx) / fx,  ry = ((float)y - cy) / fy
 *   wA = (rx * nAx + ry * nAy) + nAz,  likewise wB and wC;  s = (wA + wB) + wC
 *   det > 0: the face hits when wA >= 0, wB >= 0 and wC >= 0;  det < 0: when all three are <= 0
 *   in either case s != 0, and z = det / s must be finite with z >= near.
 * This is ray casting WITHOUT clipping: the ray (rx, ry, 1) of the pixel centre meets the face's plane at depth z along the camera's
 * axis, inside the triangle; a face that crosses z = near, or the camera's plane, is hit wherever the hit point itself is at z >= near.
 *
 * The pixel.  key = (bits of z) << 32 | f, an unsigned 64-bit word; the pixel keeps the LEAST key over all hitting faces: the least
 * depth and, on equal depths, the smallest face index.  out_depth is that z and out_face that f; a pixel nothing hits gets 0 and -1.
 * z is positive and finite, so its bits order as its value; a minimum does not depend on the order of arrival, so the image is the
 * same on every run.
 *
 * Two properties follow, and the tests check both.
 *   (1) The box is part of the definition, so how the kernels split the work cannot change a result: a face whose box holds at most
 *       HSR_MESH_DEPTH_SMALL_BOX pixels is rasterized by the lane that set it up; a larger one is appended to a list in the scratch
 *       and its box is swept by whole workgroups, 256 pixels at a time.  Both run the same hit test on the same pixels and take the
 *       same minimum.  (The constant is a speed choice, EXPERIMENTS.md §21.)
 *   (2) Two faces that share an edge leave no hole along it, whatever their winding and whichever slot the edge has in each.  For
 *       the shared corners P, Q one face evaluates w = r . cross(P, Q) and the other the same or r . cross(Q, P); cross(P, Q) is
 *       EXACTLY -cross(Q, P) in float32 (each component is the same two products subtracted the other way round), and
 *       (rx * n0 + ry * n1) + n2 negates exactly with n.  So w is the same number on both sides, with the sign each side's own
 *       orientation gives it, and a pixel centre that is outside one face by this edge (w on the wrong side of 0) is inside the
 *       other by it; a centre with w = 0 belongs to both.
 *
 * The pixel update is a 64-bit atomic minimum at agent scope whose result is not used; a plain load before it skips the atomic when
 * the new key is not smaller (the word only ever decreases, so a stale read costs one needless atomic, never a wrong result).  Every
 * loop has a bound that can be read from the code: the lane's by HSR_MESH_DEPTH_SMALL_BOX, the sweep's by H * W / 256 steps a face.
 * No workgroup waits for another and nothing spins.  The entry point sets the key image to all ones and the counter to 0 on the stream
 * first, so a scratch carries nothing from one call to the next.
 *
 * Refused: V < 1; F < 0; H or W outside 1..HSR_MESH_MAX_IMAGE_SIDE; near not finite or not positive; fx or fy not finite or zero; cx
 * or cy not finite; a NULL w2c, out_depth, out_face or scratch; a NULL vertices or faces with F > 0; scratch_bytes below
 * hsr_mesh_depth_scratch_bytes(F, H, W); a scratch that is not 16-byte aligned.  F = 0 writes the empty image.
 */
#ifndef HSR_MESH_DEPTH_H_INCLUDED
#define HSR_MESH_DEPTH_H_INCLUDED

#include <stddef.h>

#ifndef HSR_MESH_MAX_IMAGE_SIDE
#define HSR_MESH_MAX_IMAGE_SIDE 16384
#endif
#define HSR_MESH_DEPTH_SMALL_BOX 255

#ifdef __cplusplus
extern "C" {
#endif

size_t hsr_mesh_depth_scratch_bytes(int F, int H, int W);

int hsr_mesh_depth(int V, int F, const float* vertices, const int* faces, int H, int W, float fx, float fy, float cx, float cy,
                   const float* w2c, float near, void* scratch, size_t scratch_bytes, float* out_depth, int* out_face, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MESH_DEPTH_H_INCLUDED */
