"""Reading a Replica-layout sequence directory into the raw host arrays hsr_utils.frames.ingest_frame takes (host only: PIL, numpy,
json; nothing here touches the device or the library).  The layout is the one datasets/gradslam_datasets/replica.py reads (:121-124,
:331-350):

    <basedir>/<sequence>/results/frame*.jpg          colour, 8 bit
    <basedir>/<sequence>/results/depth*.png          depth, 16 bit, in units of 1 / png_depth_scale metres
    <basedir>/<sequence>/traj.txt                    one line of 16 floats per frame: the 4x4 camera-to-world matrix, row by row
    <semantic_dir>/<sequence>/semantic_class/semantic_class_*.png       optional: one raw class-id image per frame
    <semantic_dir>/<sequence>/info_semantic_tree.json                   optional: read by tree_annotation

FILE ORDER: the reference sorts its file lists with natsort.  Here the rule is stated: the files of a pattern are ordered by the
tuple of the integers that the digit runs of their base name spell (frame9.jpg before frame10.jpg, frame000123.jpg after
frame000099.jpg), ties by the name itself.  For names that differ only in one number, which is every name of this layout, that is
natsort's order.

    ReplicaSequence(basedir, sequence, start=0, end=-1, stride=1, semantic_dir=None)
        len(seq), seq[i] -> (color uint8 [H,W,3], depth uint16 [H,W], labels | None, gt_w2c float32 [4,4])
    tree_annotation(path, num_levels) -> (label_mapping_tree, num_semantic)

the Replica-V2 layout of the same file's ReplicaV2Dataset (:439-514), whose second trajectory is the held-out split of the
novel-view evaluation (hsr_utils.evaluate.evaluate_novel_views):

    <basedir>/<sequence>/imap/00/rgb/rgb_*.png, depth/depth_*.png, traj_w_c.txt      the training trajectory
    <basedir>/<sequence>/imap/01/...                                                 the test trajectory, same layout

    ReplicaV2Sequence(basedir, sequence, use_train_split=True, start=0, end=-1, stride=1)
        len(seq), seq[i] -> (color uint8 [H,W,3], depth uint16 [H,W], None, gt_w2c float32 [4,4])

and the ScanNet layout of datasets/gradslam_datasets/scannet.py (:404-418, :114), whose three images have sizes of their own
(hsr_utils.frames.ingest_frame_planes):

    <basedir>/<sequence>/color/*.jpg, depth/*.png, pose/*.txt, label-filt/*.png

    ScanNetSequence(basedir, sequence, start=0, end=-1, stride=1, labels=True)
        len(seq), seq[i] -> (color uint8 [Hc,Wc,3], depth uint16 [Hd,Wd], labels int32 [Hl,Wl] | None, gt_w2c float32 [4,4])
    scannet_class_mapping(tsv_path, column=4) -> {raw id: NYU40 id}
    scannet_tree_annotation(tsv_path, num_levels, key_column) -> (label_mapping_tree, num_semantic)

and the TUM RGB-D layout of datasets/gradslam_datasets/tum.py (:44-158), whose colour and depth images and poses are three lists with
timestamps of their own, and whose colour image is distorted (hsr_utils.frames.ingest_frame_undistort; the calibration is the
caller's, as the camera is for every reader here):

    <basedir>/<sequence>/rgb.txt, depth.txt          one "timestamp path" line per image, the path relative to the sequence
    <basedir>/<sequence>/groundtruth.txt             one "timestamp tx ty tz qx qy qz qw" line per pose; else pose.txt, the same

    TUMSequence(basedir, sequence, start=0, end=-1, stride=1, max_dt=0.08, frame_rate=32)
        len(seq), seq[i] -> (color uint8 [H,W,3], depth uint16 [H,W], None, gt_w2c float32 [4,4])

Other datasets, cropping, image pyramids and embeddings are not read.
"""
import csv
import glob
import json
import os
import re

import numpy as np


def numeric_order(paths):
    """`paths` ordered by the integers in their base names (module docstring, FILE ORDER)"""
    return sorted(paths, key=lambda p: (tuple(int(d) for d in re.findall(r"\d+", os.path.basename(p))), os.path.basename(p)))


def _read_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def _pose_lines(path, count):
    """the first `count` lines of a trajectory file as float64 [4,4] camera-to-world matrices, row by row"""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) < count:
        raise RuntimeError("hsr_utils.sequence: %s has %d poses for %d frames" % (path, len(lines), count))
    poses = []
    for i in range(count):
        values = [float(v) for v in lines[i].split()]
        if len(values) != 16:
            raise RuntimeError("hsr_utils.sequence: %s line %d has %d numbers, not 16" % (path, i + 1, len(values)))
        poses.append(np.array(values, dtype=np.float64).reshape(4, 4))
    return poses


class ReplicaSequence:
    """The retained frames [start:end:stride] of one sequence (basedataset.py:176-190: end == -1 means all; start < 0 or an end that
    is neither -1 nor beyond start is a ValueError, as there).  seq[i] decodes frame i of the retained ones and returns raw host
    arrays: colour uint8 [H,W,3], depth uint16 [H,W], the class-id image (the PNG's own integer dtype) or None without semantic_dir,
    and gt_w2c, the world-to-camera matrix relative to the first RETAINED frame: inverse(inverse(c2w_first) @ c2w_i), the reference's
    _preprocess_poses (basedataset.py:258-276) followed by the inverse of scripts/hierslam.py:1775, computed in float64 and returned
    as float32.  traj.txt has one line per frame of the directory, before [start:end:stride] is taken."""

    def __init__(self, basedir, sequence, start=0, end=-1, stride=1, semantic_dir=None):
        start, end, stride = int(start), int(end), int(stride)
        _check_range(start, end, stride)
        self.input_folder = os.path.join(basedir, sequence)
        color = numeric_order(glob.glob(os.path.join(glob.escape(self.input_folder), "results", "frame*.jpg")))
        depth = numeric_order(glob.glob(os.path.join(glob.escape(self.input_folder), "results", "depth*.png")))
        if not color or len(color) != len(depth):
            raise RuntimeError("hsr_utils.sequence: %s/results holds %d frame*.jpg and %d depth*.png files" % (self.input_folder, len(color), len(depth)))
        poses = _pose_lines(os.path.join(self.input_folder, "traj.txt"), len(color))
        semantic = None
        if semantic_dir is not None:
            folder = os.path.join(semantic_dir, sequence)
            semantic = numeric_order(glob.glob(os.path.join(glob.escape(folder), "semantic_class", "semantic_class_*.png")))
            if len(semantic) != len(color):
                raise RuntimeError("hsr_utils.sequence: %s/semantic_class holds %d images for %d frames" % (folder, len(semantic), len(color)))
        stop = len(color) if end == -1 else end
        pick = slice(start, stop, stride)
        self.color_paths, self.depth_paths = color[pick], depth[pick]
        self.semantic_paths = None if semantic is None else semantic[pick]
        self.retained_inds = list(range(len(color)))[pick]
        self.c2w = poses[pick]
        if not self.color_paths:
            raise RuntimeError("hsr_utils.sequence: no frame of %d left by start=%d, end=%d, stride=%d" % (len(color), start, end, stride))
        self._first_inv = np.linalg.inv(self.c2w[0])

    def __len__(self):
        return len(self.color_paths)

    def gt_w2c(self, i):
        rel_c2w = self._first_inv @ self.c2w[i]
        return np.linalg.inv(rel_c2w).astype(np.float32)

    def __getitem__(self, i):
        i = range(len(self))[i]      # negative indices; IndexError beyond the end, so that iteration stops
        color = _read_image(self.color_paths[i])
        depth = _read_image(self.depth_paths[i])
        if color.dtype != np.uint8 or color.ndim != 3 or color.shape[2] != 3:
            raise RuntimeError("hsr_utils.sequence: %s is not an 8-bit three-channel image (%s %s)" % (self.color_paths[i], color.dtype, color.shape))
        if depth.ndim != 2 or depth.shape != color.shape[:2]:
            raise RuntimeError("hsr_utils.sequence: %s is not a one-channel image of the colour image's size (%s)" % (self.depth_paths[i], depth.shape))
        if depth.dtype != np.uint16:      # PIL decodes a 16-bit grey PNG as int32 ('I') or uint16 ('I;16'), by version; the values are 0..65535
            if depth.min() < 0 or depth.max() > 65535:
                raise RuntimeError("hsr_utils.sequence: %s holds values outside 16 bits" % self.depth_paths[i])
            depth = depth.astype(np.uint16)
        labels = None
        if self.semantic_paths is not None:
            labels = _read_image(self.semantic_paths[i])
            if labels.ndim != 2 or labels.shape != depth.shape or labels.dtype.kind not in "iu":
                raise RuntimeError("hsr_utils.sequence: %s is not a one-channel integer image of the frame's size (%s %s)" % (
                    self.semantic_paths[i], labels.dtype, labels.shape))
        return np.ascontiguousarray(color), np.ascontiguousarray(depth), labels, self.gt_w2c(i)


class ReplicaV2Sequence(ReplicaSequence):
    """The retained frames [start:end:stride] of one Replica-V2 sequence, as the reference's ReplicaV2Dataset reads it
    (datasets/gradslam_datasets/replica.py:439-514), in numeric_order:

        use_train_split=True    <basedir>/<sequence>/imap/00/rgb/rgb_*.png, depth/depth_*.png and traj_w_c.txt (one line of 16 floats per
                                frame: the camera-to-world matrix, row by row)
        use_train_split=False   the same from imap/01, with the FIRST TRAINING FRAME (imap/00/rgb/rgb_0.png, depth/depth_0.png and line 1
                                of imap/00/traj_w_c.txt) put in front (:483-486, :494-500): item 0 is that frame, item i >= 1 is test view
                                i - 1, which is the order hsr_utils.evaluate.evaluate_novel_views reads.  [start:end:stride] is taken of
                                that list, as the reference's base class does.

    Items, checks and errors are ReplicaSequence's: raw host arrays (colour uint8 [H,W,3], depth uint16 [H,W], None for the labels,
    which this layout does not have) and gt_w2c relative to the first RETAINED frame, inverse(inverse(c2w_first) @ c2w_i) in float64,
    returned as float32 — for the test split with start=0 that is relative to the first training frame, the frame the map's poses are
    relative to."""

    def __init__(self, basedir, sequence, use_train_split=True, start=0, end=-1, stride=1):
        start, end, stride = int(start), int(end), int(stride)
        _check_range(start, end, stride)
        self.use_train_split = bool(use_train_split)
        train_folder = os.path.join(basedir, sequence, "imap", "00")
        self.input_folder = train_folder if self.use_train_split else os.path.join(basedir, sequence, "imap", "01")
        folder = glob.escape(self.input_folder)
        color = numeric_order(glob.glob(os.path.join(folder, "rgb", "rgb_*.png")))
        depth = numeric_order(glob.glob(os.path.join(folder, "depth", "depth_*.png")))
        if not color or len(color) != len(depth):
            raise RuntimeError("hsr_utils.sequence: %s holds %d rgb/rgb_*.png and %d depth/depth_*.png files" % (self.input_folder, len(color), len(depth)))
        poses = _pose_lines(os.path.join(self.input_folder, "traj_w_c.txt"), len(color))
        if not self.use_train_split:
            first = (os.path.join(train_folder, "rgb", "rgb_0.png"), os.path.join(train_folder, "depth", "depth_0.png"))
            for path in first:
                if not os.path.exists(path):
                    raise RuntimeError("hsr_utils.sequence: %s, the first training frame, is missing" % path)
            color, depth = [first[0]] + color, [first[1]] + depth
            poses = _pose_lines(os.path.join(train_folder, "traj_w_c.txt"), 1) + poses
        stop = len(color) if end == -1 else end
        pick = slice(start, stop, stride)
        self.color_paths, self.depth_paths = color[pick], depth[pick]
        self.semantic_paths = None
        self.retained_inds = list(range(len(color)))[pick]
        self.c2w = poses[pick]
        if not self.color_paths:
            raise RuntimeError("hsr_utils.sequence: no frame of %d left by start=%d, end=%d, stride=%d" % (len(color), start, end, stride))
        self._first_inv = np.linalg.inv(self.c2w[0])


def _tum_list(path, columns):
    """the lines of a TUM list file that do not start with '#', split at blanks: [[cell, ...], ...], each of at least `columns` cells"""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f.read().splitlines()):
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            cells = line.split()
            if len(cells) < columns:
                raise RuntimeError("hsr_utils.sequence: %s line %d has %d cells, not %d" % (path, n + 1, len(cells), columns))
            rows.append(cells)
    if not rows:
        raise RuntimeError("hsr_utils.sequence: %s lists nothing" % path)
    return rows


def quaternion_c2w(values):
    """float64 [4,4] camera-to-world matrix of one TUM pose (tx, ty, tz, qx, qy, qz, qw): the quaternion, scalar LAST, is normalised
    first, as scipy's Rotation.from_quat does for the reference (tum.py:69-76)"""
    tx, ty, tz, x, y, z, w = (float(v) for v in values)
    norm = np.sqrt(x * x + y * y + z * z + w * w)
    if not np.isfinite(norm) or norm == 0.0:
        raise RuntimeError("hsr_utils.sequence: a pose's quaternion (%r, %r, %r, %r) has no direction" % (x, y, z, w))
    x, y, z, w = x / norm, y / norm, z / norm, w / norm
    pose = np.eye(4, dtype=np.float64)
    pose[:3, :3] = [[x * x - y * y - z * z + w * w, 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                    [2.0 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2.0 * (y * z - x * w)],
                    [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), -x * x - y * y + z * z + w * w]]
    pose[:3, 3] = (tx, ty, tz)
    return pose


class TUMSequence(ReplicaSequence):
    """The retained frames [start:end:stride] of one TUM RGB-D sequence, as the reference's TUMDataset reads it
    (datasets/gradslam_datasets/tum.py:44-158):

      lists        rgb.txt, depth.txt and groundtruth.txt (pose.txt when there is no groundtruth.txt); a line that starts with '#' is
                   ignored (the reference's np.loadtxt drops them too, and its skiprows=1 on the pose list drops one more comment line
                   of the dataset's three);
      association  for each colour timestamp t, in the order of rgb.txt, the depth line and the pose line whose timestamps are
                   nearest to t (the first of equally near ones); the triple is kept when BOTH are closer than max_dt seconds
                   (|dt| < max_dt; tum.py:50-67);
      thinning     the first triple is kept; every other one when its colour timestamp is more than 1 / frame_rate seconds after
                   that of the last KEPT triple (tum.py:101-106; frame_rate is the reference's constant 32);
      poses        t tx ty tz qx qy qz qw, camera to world, the quaternion normalised (quaternion_c2w: plain numpy).

    [start:end:stride] is then taken of the thinned list, with ReplicaSequence's rules and errors; `retained_inds` indexes that list
    and `associations` holds the (colour line, depth line, pose line) of every retained frame.  seq[i] returns raw host arrays: colour
    uint8 [H,W,3], depth uint16 [H,W] (TUM's png_depth_scale is 5000), None for the labels, which this layout does not have, and
    gt_w2c float32 [4,4] relative to the first RETAINED frame: inverse(inverse(c2w_first) @ c2w_i) in float64, as the other readers
    (the reference rounds each pose to float32 first, tum.py:155).  The calibration, distortion included, is the caller's:
    SlamSession.ingest(..., undistort=(fx, fy, cx, cy, coefficients))."""

    def __init__(self, basedir, sequence, start=0, end=-1, stride=1, max_dt=0.08, frame_rate=32):
        start, end, stride = int(start), int(end), int(stride)
        _check_range(start, end, stride)
        max_dt, frame_rate = float(max_dt), float(frame_rate)
        if not max_dt > 0.0 or not frame_rate > 0.0:
            raise ValueError("hsr_utils.sequence: max_dt and frame_rate must be positive; got %r, %r" % (max_dt, frame_rate))
        self.input_folder = os.path.join(basedir, sequence)
        for name in ("rgb.txt", "depth.txt"):
            if not os.path.isfile(os.path.join(self.input_folder, name)):
                raise RuntimeError("hsr_utils.sequence: %s has no %s" % (self.input_folder, name))
        self.pose_path = next((p for p in (os.path.join(self.input_folder, n) for n in ("groundtruth.txt", "pose.txt")) if os.path.isfile(p)), None)
        if self.pose_path is None:
            raise RuntimeError("hsr_utils.sequence: %s has neither groundtruth.txt nor pose.txt" % self.input_folder)
        images = _tum_list(os.path.join(self.input_folder, "rgb.txt"), 2)
        depths = _tum_list(os.path.join(self.input_folder, "depth.txt"), 2)
        poses = _tum_list(self.pose_path, 8)
        t_image = np.array([float(r[0]) for r in images], dtype=np.float64)
        t_depth = np.array([float(r[0]) for r in depths], dtype=np.float64)
        t_pose = np.array([float(r[0]) for r in poses], dtype=np.float64)
        triples = []
        for i, t in enumerate(t_image):
            j, k = int(np.argmin(np.abs(t_depth - t))), int(np.argmin(np.abs(t_pose - t)))
            if abs(t_depth[j] - t) < max_dt and abs(t_pose[k] - t) < max_dt:
                triples.append((i, j, k))
        if not triples:
            raise RuntimeError("hsr_utils.sequence: %s: no colour image has a depth image and a pose within %g s" % (self.input_folder, max_dt))
        kept = [triples[0]]
        for triple in triples[1:]:
            if t_image[triple[0]] - t_image[kept[-1][0]] > 1.0 / frame_rate:
                kept.append(triple)
        stop = len(kept) if end == -1 else end
        pick = slice(start, stop, stride)
        self.associations = kept[pick]
        self.retained_inds = list(range(len(kept)))[pick]
        if not self.associations:
            raise RuntimeError("hsr_utils.sequence: no frame of %d left by start=%d, end=%d, stride=%d" % (len(kept), start, end, stride))
        self.color_paths = [os.path.join(self.input_folder, images[i][1]) for i, _j, _k in self.associations]
        self.depth_paths = [os.path.join(self.input_folder, depths[j][1]) for _i, j, _k in self.associations]
        self.semantic_paths = None
        self.timestamps = [float(t_image[i]) for i, _j, _k in self.associations]
        self.c2w = [quaternion_c2w(poses[k][1:8]) for _i, _j, k in self.associations]
        self._first_inv = np.linalg.inv(self.c2w[0])


def tree_annotation(path, num_levels):
    """info_semantic_tree.json as the reference reads it (replica.py:630-691 with :144-147).  The file is a dict whose keys are
    "<class id>_<class name>" and whose values list, level by level from the root, one {"<level label>": "<name>"} dict per level
    the class has.  Returns (label_mapping_tree, num_semantic):
      label_mapping_tree  {class id as the key's str: tuple of num_levels level labels}, -1 where the class has fewer levels; in the
                          file's order (what frames.tree_label_table and evaluate.tree_lookup_table take);
      num_semantic        the classes per level, the largest label of the level + 1, with the number of classes of the file appended
                          (the reference's find_max_level(flag_add=True) plus len(label_mapping_tree))."""
    L = int(num_levels)
    with open(path) as f:
        annotations = json.load(f)
    tree = {}
    for key, item in annotations.items():
        base_id = key.split("_")[0]
        int(base_id)      # a key that does not begin with a class id is an error, as in the reference
        if len(item) > L:
            raise RuntimeError("hsr_utils.sequence: class %r has %d levels, num_levels is %d" % (key, len(item), L))
        levels = [-1] * L
        for i_level, level_info in enumerate(item):
            for label in level_info:      # one entry per level; of several the last one stays
                levels[i_level] = int(label)
        tree[base_id] = tuple(levels)
    if not tree:
        raise RuntimeError("hsr_utils.sequence: %s names no class" % path)
    columns = np.asarray(list(tree.values()), dtype=np.int64)
    num_semantic = [int(columns[:, i].max()) + 1 for i in range(L)] + [len(tree)]
    return tree, num_semantic


def _check_range(start, end, stride):
    """the [start:end:stride] rules of ReplicaSequence (basedataset.py:176-190)"""
    if start < 0:
        raise ValueError("hsr_utils.sequence: start must not be negative; got %d" % start)
    if not (end == -1 or end > start):
        raise ValueError("hsr_utils.sequence: end (%d) must be -1 (all frames) or greater than start (%d)" % (end, start))
    if stride < 1:
        raise ValueError("hsr_utils.sequence: stride must be at least 1; got %d" % stride)


def _as_uint16(image, path):
    """PIL decodes a 16-bit grey PNG as int32 ('I') or uint16 ('I;16'), by version; the values are 0..65535"""
    if image.dtype != np.uint16:
        if image.dtype.kind not in "iu" or image.min() < 0 or image.max() > 65535:
            raise RuntimeError("hsr_utils.sequence: %s holds values outside 16 bits" % path)
        image = image.astype(np.uint16)
    return image


class ScanNetSequence:
    """The retained frames [start:end:stride] of one ScanNet-layout sequence, as datasets/gradslam_datasets/scannet.py reads it
    (:404-418, :114), in numeric_order:

        <basedir>/<sequence>/color/*.jpg          colour, 8 bit (968x1296 in the dataset)
        <basedir>/<sequence>/depth/*.png          depth, 16 bit, in millimetres (480x640; png_depth_scale 1000)
        <basedir>/<sequence>/pose/*.txt           one 4x4 camera-to-world matrix per file, row by row
        <basedir>/<sequence>/label-filt/*.png     raw ScanNet class ids, 16 bit (968x1296); read unless labels=False

    seq[i] decodes frame i of the retained ones and returns raw host arrays: colour uint8 [Hc,Wc,3], depth uint16 [Hd,Wd], the
    class-id image int32 [Hl,Wl] (None with labels=False) and gt_w2c float32 [4,4].  The three images may differ in size: they are what
    frames.ingest_frame_planes and SlamSession.ingest take.  The start / end / stride rules, the errors and `retained_inds` are
    ReplicaSequence's, and gt_w2c is, as there, relative to the first RETAINED frame: inverse(inverse(c2w_first) @ c2w_i) in float64,
    returned as float32.  ScanNet marks a frame whose pose was lost with a matrix of -inf: a pose file that holds a non-finite number
    gives its frame a gt_w2c full of NaN, and SlamSession.step keeps such a frame out of the keyframes, as the reference's check at
    scripts/hierslam.py:2108-2109 does.  A non-finite FIRST retained pose (every other pose is relative to it) is a RuntimeError
    naming the file.  Pyramids and embeddings are not read."""

    def __init__(self, basedir, sequence, start=0, end=-1, stride=1, labels=True):
        start, end, stride = int(start), int(end), int(stride)
        _check_range(start, end, stride)
        self.input_folder = os.path.join(basedir, sequence)
        folder = glob.escape(self.input_folder)
        color = numeric_order(glob.glob(os.path.join(folder, "color", "*.jpg")))
        depth = numeric_order(glob.glob(os.path.join(folder, "depth", "*.png")))
        pose = numeric_order(glob.glob(os.path.join(folder, "pose", "*.txt")))
        if not color or len(color) != len(depth):
            raise RuntimeError("hsr_utils.sequence: %s holds %d color/*.jpg and %d depth/*.png files" % (self.input_folder, len(color), len(depth)))
        if len(pose) < len(color):
            raise RuntimeError("hsr_utils.sequence: %s/pose has %d poses for %d frames" % (self.input_folder, len(pose), len(color)))
        semantic = None
        if labels:
            semantic = numeric_order(glob.glob(os.path.join(folder, "label-filt", "*.png")))
            if len(semantic) != len(color):
                raise RuntimeError("hsr_utils.sequence: %s/label-filt holds %d images for %d frames" % (self.input_folder, len(semantic), len(color)))
        stop = len(color) if end == -1 else end
        pick = slice(start, stop, stride)
        self.color_paths, self.depth_paths, self.pose_paths = color[pick], depth[pick], pose[:len(color)][pick]
        self.label_paths = None if semantic is None else semantic[pick]
        self.retained_inds = list(range(len(color)))[pick]
        if not self.color_paths:
            raise RuntimeError("hsr_utils.sequence: no frame of %d left by start=%d, end=%d, stride=%d" % (len(color), start, end, stride))
        self.c2w = []
        for path in self.pose_paths:
            with open(path) as f:
                values = [float(v) for v in f.read().split()]
            if len(values) != 16:
                raise RuntimeError("hsr_utils.sequence: %s has %d numbers, not 16" % (path, len(values)))
            self.c2w.append(np.array(values, dtype=np.float64).reshape(4, 4))
        if not np.isfinite(self.c2w[0]).all():
            raise RuntimeError("hsr_utils.sequence: %s, the first retained pose, is not finite; every other pose is relative to it" % self.pose_paths[0])
        self._first_inv = np.linalg.inv(self.c2w[0])

    def __len__(self):
        return len(self.color_paths)

    def gt_w2c(self, i):
        if not np.isfinite(self.c2w[i]).all():
            return np.full((4, 4), np.nan, dtype=np.float32)
        return np.linalg.inv(self._first_inv @ self.c2w[i]).astype(np.float32)

    def __getitem__(self, i):
        i = range(len(self))[i]      # negative indices; IndexError beyond the end, so that iteration stops
        color = _read_image(self.color_paths[i])
        depth = _read_image(self.depth_paths[i])
        if color.dtype != np.uint8 or color.ndim != 3 or color.shape[2] != 3:
            raise RuntimeError("hsr_utils.sequence: %s is not an 8-bit three-channel image (%s %s)" % (self.color_paths[i], color.dtype, color.shape))
        if depth.ndim != 2:
            raise RuntimeError("hsr_utils.sequence: %s is not a one-channel image (%s)" % (self.depth_paths[i], depth.shape))
        depth = _as_uint16(depth, self.depth_paths[i])
        labels = None
        if self.label_paths is not None:
            labels = _read_image(self.label_paths[i])
            if labels.ndim != 2 or labels.dtype.kind not in "iu":
                raise RuntimeError("hsr_utils.sequence: %s is not a one-channel integer image (%s %s)" % (self.label_paths[i], labels.dtype, labels.shape))
            labels = np.ascontiguousarray(labels.astype(np.int32))
        return np.ascontiguousarray(color), np.ascontiguousarray(depth), labels, self.gt_w2c(i)


def _tsv_rows(tsv_path):
    """the tab-separated cells of every line after the header line"""
    with open(tsv_path, newline="") as f:
        return [row for i, row in enumerate(csv.reader(f, delimiter="\t")) if i > 0 and row]


def scannet_class_mapping(tsv_path, column=4):
    """scannetv2-labels.combined.tsv as the reference's load_scannet_nyu40_mapping reads it (scannet.py:575-599): the header line is
    skipped and every other line gives {int(cell 0): int(cell `column`)} — the raw ScanNet id to the NYU40 id with column 4.  Of two
    lines with one id the later wins.  What frames.composed_label_table takes as class_mapping."""
    mapping = {}
    for n, row in enumerate(_tsv_rows(tsv_path)):
        if len(row) <= column:
            raise RuntimeError("hsr_utils.sequence: %s line %d has %d cells, column %d is wanted" % (tsv_path, n + 2, len(row), column))
        mapping[int(row[0])] = int(row[column])
    return mapping


def scannet_tree_annotation(tsv_path, num_levels, key_column):
    """The tree tsv of the reference's ScanNet configs.  RESTATED, NOT PINNED BY A FILE OF THE DATASET: no tree tsv file is among this
    project's fixtures, and the format is taken from the reference's two readers, scannet.py:734-795 (key_column=4, the NYU40 id;
    four levels) and :890-966 (key_column=0, the raw id; five levels).  The header line is skipped.  On every other line the key is int(cell key_column) and
    level l's label is int(cell 17 + 2l), the cell after it holding the level's name; an empty cell, or one the line is too short
    to have, is -1 (the reference keeps None there).  Of two lines with one key the later wins.  Returns (label_mapping_tree,
    num_semantic) shaped like tree_annotation's: {key: tuple of num_levels labels} in ascending key order (the reference sorts), and
    the largest label of each level + 1 followed by the number of keys."""
    L = int(num_levels)
    if L < 1:
        raise ValueError("hsr_utils.sequence: scannet_tree_annotation takes at least one level, not %d" % L)
    tree = {}
    for n, row in enumerate(_tsv_rows(tsv_path)):
        if len(row) <= key_column:
            raise RuntimeError("hsr_utils.sequence: %s line %d has %d cells, key column %d is wanted" % (tsv_path, n + 2, len(row), key_column))
        cells = [row[17 + 2 * l] if 17 + 2 * l < len(row) else "" for l in range(L)]
        tree[int(row[key_column])] = tuple(int(c) if c != "" else -1 for c in cells)
    if not tree:
        raise RuntimeError("hsr_utils.sequence: %s names no class" % tsv_path)
    tree = dict(sorted(tree.items()))
    columns = np.asarray(list(tree.values()), dtype=np.int64)
    num_semantic = [int(columns[:, i].max()) + 1 for i in range(L)] + [len(tree)]
    return tree, num_semantic


__all__ = ["ReplicaSequence", "ReplicaV2Sequence", "tree_annotation", "numeric_order", "ScanNetSequence", "scannet_class_mapping", "scannet_tree_annotation",
           "TUMSequence"]
