/*
 * hsr_map_export.h — C ABI of the device export of the Gaussian map as the body of a PLY file (libhsr_rast.so), DESIGN.md §7 row 10:
 * what the reference's scripts/export_ply_semantic_tree.py does between the arrays of params.npz and PlyData.write — save_ply :251-277,
 * save_ply_semantic :279-327 with transfer_tree_label :208-228 and semantic_label_vis :230-248, save_ply_semantic_multilevel :329-382.
 * hsr_frame_export.h's label rule, tuple table and class table turned on the map itself: the logits are row-major per Gaussian instead
 * of planar, and the output is packed PLY records.  An extension under include/ext/: the prototypes under include/hsr_*.h are a counted
 * set (tests/test_abi.py); this one is bound under its key in diff_gaussian_rasterization/_abi.py HEADERS.
 *
 * One call is ONE launch; the job struct travels by value in the kernel's arguments.  No scratch, no allocation, no host
 * synchronisation.  P = 0 succeeds and launches nothing: the checks below hold for it too, except that its pointers may be NULL, as
 * those of empty arrays are.  HSR_ERR_INVALID_ARGUMENT, and nothing launched, for:
 * job NULL; P < 0 or P > HSR_MAP_EXPORT_MAX_P (31 580 641 = floor((2^31 - 1) / 68): every byte offset into the body fits a signed 32-bit
 * int, which is what the kernel counts them in); an unknown record; record NONE without out_labels; for SH and RGB8: S not 1 or 3, a NULL
 * means3D, unnorm_rotations, logit_opacities, log_scales or out, a NULL rgb_colors for SH, an unknown colour for RGB8, a NULL colours
 * for GIVEN, a NULL labels or table or n < 1 for LABELS; where the tree is read (RGB8 with TREE, and NONE): a NULL semantic, L outside
 * 1 .. HSR_EVAL_MAX_LEVELS (16, hsr_eval.h), a level size below 1, sum(sizes) > K; and for RGB8 with TREE a NULL table, n < 1 or
 * prod(sizes) != n.  No output may overlap an input or the other output.  Fields the chosen kinds do not name are not read: `colour` and
 * what it selects for RGB8 only, rgb_colors for SH only, out_labels for RGB8 with TREE and for NONE only, table and n not for NONE.
 *
 * The records, one per Gaussian, packed without padding, every float little endian (the byte layouts tests/test_gpu_map_io.py pins for
 * the host writer hsr_utils/map_io.py):
 *   HSR_MAP_RECORD_SH    68 bytes, 17 floats: x y z  nx ny nz  f_dc_0 f_dc_1 f_dc_2  opacity  scale_0 scale_1 scale_2  rot_0 .. rot_3
 *   HSR_MAP_RECORD_RGB8  59 bytes: the same with red green blue as three bytes at offset 24 in place of f_dc_*: opacity at 27,
 *                        scale_0 at 31, rot_0 at 43
 *   HSR_MAP_RECORD_NONE  no records: `out` and the map arrays are not read; the call gives out_labels only
 * x y z = means3D[g]; nx ny nz = normals[g], or zeros (+0.0f) when normals is NULL; opacity = logit_opacities[g]; rot = unnorm_rotations[g];
 * scale_0..2 = log_scales[g] when S = 3, the one log-scale three times when S = 1 (np.tile, :259-260, :310-311).  Logits, log-scales and
 * quaternions go out as stored, as the reference writes them.  Every float but f_dc_* is a BIT COPY, NaNs with their payloads included.
 *     f_dc_c = (rgb_c - 0.5f) / C0f        one fp32 subtraction, one correctly rounded fp32 division (rgb_to_spherical_harmonic :201-202)
 * with C0f = 0.282094806f (0x3e906ebb), the fp32 nearest to 0.28209479177387814 — what numpy computes from a float32 array and the two
 * Python floats.  A NaN gives a NaN (payload not stated), +-inf itself.  The file is compiled with -ffp-contract=off; nothing here needs
 * a fused multiply-add.
 *
 * The colour of an RGB8 record:
 *   HSR_MAP_COLOUR_GIVEN   colours uint8 [P,3]: copied.
 *   HSR_MAP_COLOUR_LABELS  labels int32 [P], table uint8 [n,3]: table[label] for 0 <= label < n, else black (0, 0, 0).  The reference
 *                          indexes a numpy array (:294, :352), whose negative indices wrap to the end of the table; that wrap is
 *                          deliberately NOT copied (as hsr_frame_export.h, LABELS).
 *   HSR_MAP_COLOUR_TREE    semantic float32 [P,K] row-major, row stride K; sizes[L]; table uint8 [n,3], n = prod(sizes).  Level l owns
 *                          the columns begin_l .. begin_l + sizes[l] - 1, begin_l = sizes[0] + .. + sizes[l-1]; columns from sum(sizes)
 *                          on are not used (they may hold anything).  The label of a level is that of hsr_eval_labels_tree (hsr_eval.h)
 *                          and of hsr_frame_export.h's LOGITS, bit for bit (one definition, csrc/hsr_tree.h): with m the largest x_i of the level's columns (fmaxf from
 *                          -inf, in index order) and s the fp32 sum of expf(x_i - m) in index order, the lowest i with
 *                          expf(x_i - m) / s == 1.0f / s; 0 when there is none (a NaN or +inf among the level's values: s is then a
 *                          NaN; a -inf beside finite values is a value like any other and never wins).  The
 *                          colour is table[idx],
 *                              idx = (..((label_0 * sizes[1] + label_1) * sizes[2] + label_2)..) * sizes[L-1] + label_{L-1}
 *                          the mixed-radix index with level 0 most significant, hsr_utils.evaluate.tree_lookup_table's.
 * out_labels int32 [L,P], or NULL: label_l of Gaussian g at out_labels[l * P + g] — the device form of transfer_tree_label (:208-228).
 *
 * All pointers are DEVICE pointers except `job`, a HOST struct.  Everything runs on `stream`.  A workgroup takes 256 consecutive
 * Gaussians (128 or 64 where K is large): it reads the spans of the map arrays that belong to them flat (16 bytes per lane), stages
 * whole logit rows through LDS, assembles its records in LDS and writes their contiguous bytes (256 * 59, 256 * 68 and their halves and
 * quarters are multiples of 16) with 16-byte stores.  When
 * `out` or any array the call reads is not 16-byte aligned the whole call takes a variant of 4-byte loads and 1-byte stores with the
 * same results.  Nothing is written past out[P * stride - 1].  Errors: return <0 and hsr_last_error() (hsr_rasterizer.h).
 */
#ifndef HSR_MAP_EXPORT_H_INCLUDED
#define HSR_MAP_EXPORT_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSR_MAP_EXPORT_MAX_P 31580641
#define HSR_MAP_RECORD_SH    0   /* 68 bytes: 17 floats, the colour as f_dc_0..2                  */
#define HSR_MAP_RECORD_RGB8  1   /* 59 bytes: red green blue as bytes at offset 24                */
#define HSR_MAP_RECORD_NONE  2   /* no records: out_labels only                                   */
#define HSR_MAP_COLOUR_GIVEN  0  /* colours uint8 [P,3]                                           */
#define HSR_MAP_COLOUR_LABELS 1  /* labels int32 [P], table uint8 [n,3]                           */
#define HSR_MAP_COLOUR_TREE   2  /* semantic float [P,K], sizes[L], table uint8 [prod(sizes),3]   */

typedef struct hsr_map_export_job {
    int P;
    int S;                         /* columns of log_scales: 1 or 3 */
    int record;
    int colour;
    const float* means3D;          /* [P,3] */
    const float* rgb_colors;       /* [P,3] */
    const float* unnorm_rotations; /* [P,4] */
    const float* logit_opacities;  /* [P] */
    const float* log_scales;       /* [P,S] */
    const float* normals;          /* [P,3], or NULL for zeros */
    const uint8_t* colours;        /* [P,3] */
    const int32_t* labels;         /* [P] */
    const float* semantic;         /* [P,K] */
    const uint8_t* table;          /* [n,3], rows R G B */
    int n;
    int K, L;
    int sizes[16];                 /* 16 = HSR_EVAL_MAX_LEVELS */
    uint8_t* out;                  /* [P * stride] */
    int32_t* out_labels;           /* [L,P], or NULL */
} hsr_map_export_job;

/* job: HOST struct */
int hsr_map_export(const hsr_map_export_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_MAP_EXPORT_H_INCLUDED */
