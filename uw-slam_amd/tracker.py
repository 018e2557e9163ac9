"""Host-side mirror of the reference's Tracker / LS / Frame surface for the direct-tracking path, over the C ABI.

Same method names, argument meaning and call order as include/Tracker.h:97-170, include/LeastSquares.h:31-45 and
the Frame fields of include/System.h:85-100 that the path touches, so that System::Tracking()'s sequence
(src/System.cpp:193-223) reads the same here:

    tracker = Tracker(depth_available); tracker.InitializePyramid(w, h, K)
    tracker.ApplyGradient(prev); tracker.ApplyGradient(cur)
    tracker.ObtainAllPoints(prev)
    tracker.EstimatePose(prev, cur)     # -> prev.rigid_transformation_

Everything numeric happens in libuwt_hip.so; this file only moves buffers.  (The compiled-language mirror for C++
callers is include/uw_tracker.hpp.)
"""
import numpy as np

from . import capi

PYRAMID_LEVELS = 5  # src/Options.cpp:26


class Frame:
    """include/System.h:63-103 — only the members the tracker reads or writes."""

    def __init__(self, image, depth=None, id_frame=0):
        self.idFrame_ = id_frame
        self.images_ = [np.ascontiguousarray(image, np.uint8)]
        self.depths_ = [np.ascontiguousarray(depth, np.uint16)] if depth is not None else []
        self.depth_available_ = depth is not None
        self.obtained_gradients_ = False
        self.obtained_candidatePoints_ = False
        self.rigid_transformation_ = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)  # qx qy qz qw tx ty tz
        self.keypoints_ = np.zeros((0, 2), np.float32)       # cv::KeyPoint::pt of Frame::keypoints_
        self.n_matches_ = 0                                  # include/System.h:93
        self.surf_keypoints_ = np.zeros(0, capi.KEYPOINT)    # the same key points as cv::KeyPoint holds them (size, response, direction,
                                                             # octave): what useProvidedKeypoints describes again in the next call
        self.orb_keypoints_ = np.zeros(0, capi.KEYPOINT)     # the same under RobustMatcher(detector=1): ORB's records
        self.candidatePoints_ = {}                           # level -> N x 4 [x y z w] when a sparse producer ran
        self._slot = None


class Tracker:
    """include/Tracker.h:90-170.  Solver constants are the locals of Tracker::EstimatePose (src/Tracker.cpp:364-372)
    unless overridden through **params (the uwt_params fields)."""

    def __init__(self, _depth_available=False, max_frames=16, device=0, **params):
        self.depth_available_ = bool(_depth_available)
        self._max_frames = max(2, int(max_frames))   # an alignment binds two frames at once (uw::Tracker clamps the same way)
        self._device = device
        self._over = params
        self._ctx = None
        self._owner = [None] * self._max_frames          # slot -> Frame holding it
        self._last_use = [0] * self._max_frames
        self._clock = 0

    def InitializePyramid(self, _width, _height, _K):
        K = np.asarray(_K, np.float32)
        over = dict(n_levels=PYRAMID_LEVELS, max_frames=self._max_frames, max_pairs=max(1, self._max_frames // 2),
                    has_depth=int(self.depth_available_), device=self._device)
        over.update(self._over)
        p = capi.default_params(int(_width), int(_height), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), **over)
        # (UwtError for parameters uwt_create refuses; with depth: a depth_scale whose depths leave [capi.DEPTH_MIN, capi.DEPTH_MAX])
        self._ctx = capi.Context(p)
        if LS._default_ctx is None or not LS._default_ctx._h:
            LS.bind(self._ctx)                  # `LS ls;` inside the tracking loop folds on the tracker's context
        self._ctx.set_deferred(True)   # one wait per frame, in EstimatePose (pyramids and gradients are enqueued only)
        lv = [self._ctx.level_info(l) for l in range(p.n_levels)]
        self.w_ = [L.w for L in lv]
        self.h_ = [L.h for L in lv]
        self.fx_ = [L.fx for L in lv]
        self.fy_ = [L.fy for L in lv]
        self.cx_ = [L.cx for L in lv]
        self.cy_ = [L.cy for L in lv]
        self.invfx_ = [L.invfx for L in lv]
        self.invfy_ = [L.invfy for L in lv]

    def InitializeMasks(self):
        """src/Tracker.cpp:342-359 builds masks nothing reads; kept as a no-op for call-order compatibility."""

    def _bind(self, frame):
        """System::AddFrame's pyramid loop (src/System.cpp:246-251): upload level 0, build levels 1.. on the GPU."""
        self._clock += 1
        if frame._slot is not None and self._owner[frame._slot] is frame:
            self._last_use[frame._slot] = self._clock
            return frame._slot
        # least-recently-used slot; the frame that held it is told (it uploads again when next used, and its gradients
        # are gone) instead of silently reading another frame's planes
        free = [i for i, o in enumerate(self._owner) if o is None]
        slot = free[0] if free else min(range(self._max_frames), key=lambda i: self._last_use[i])
        old = self._owner[slot]
        if old is not None:
            old._slot = None
            old.obtained_gradients_ = False
        self._owner[slot] = frame
        self._last_use[slot] = self._clock
        frame._slot = slot
        frame.obtained_gradients_ = False
        self._ctx.set_frame(slot, frame.images_[0], frame.depths_[0] if self.depth_available_ else None)
        self._ctx.build_pyramids(slot, 1)
        return slot

    def ApplyGradient(self, _frame):
        slot = self._bind(_frame)
        self._ctx.apply_gradient(slot, 1)
        _frame.obtained_gradients_ = True

    def ObtainAllPoints(self, _frame):
        """src/Tracker.cpp:1259-1310.  The dense table is the pixel grid; the kernels derive (x, y, z, w) in
        registers instead of materialising N x 4 floats."""
        self._bind(_frame)
        _frame.obtained_candidatePoints_ = True

    def WarpFunction(self, _points2warp, _rigid_transformation, _lvl):
        return self._ctx.warp(int(_lvl), _points2warp, _rigid_transformation)

    def EstimatePose(self, _previous_frame, _current_frame):
        a, b = self._bind(_previous_frame), self._bind(_current_frame)
        if not _previous_frame.obtained_gradients_:  # reference: empty cv::Mat
            raise RuntimeError("ApplyGradient(previous_frame) must run before EstimatePose (or its slot was reused since)")
        poses, stats = self._ctx.estimate_pose_batch([a], [b], raise_on_pair_failure=True)
        _previous_frame.rigid_transformation_ = poses[0]
        return stats[0]

    def EstimatePoseSeeded(self, _previous_frame, _current_frame, seed, handoff=0):
        """EstimatePose from a start pose (uwt_estimate_pose_batch_seeded): seed = qx qy qz qw tx ty tz, the pose in front of the first
        evaluation, used as given — a keyframe's prediction (PredictSeeds), the previous pair's pose, another stage's result.
        handoff: 0 / "reference" the reference's level hand-off, 1 / "keep" the pose crosses the levels unchanged.  A seed with a
        non-finite entry, or with |tx|, |ty| or |tz| above capi.TRANSLATION_MAX (2^125, the range of the dense warp's division), is
        refused: UwtError with ERR_PAIR_FAILED, ERR_INVALID_ARG in the pair's stats."""
        a, b = self._bind(_previous_frame), self._bind(_current_frame)
        if not _previous_frame.obtained_gradients_:
            raise RuntimeError("ApplyGradient(previous_frame) must run before EstimatePoseSeeded (or its slot was reused since)")
        poses, stats = self._ctx.estimate_pose_batch_seeded([a], [b], np.asarray(seed, np.float32).reshape(1, 7), handoff,
                                                            raise_on_pair_failure=True)
        _previous_frame.rigid_transformation_ = poses[0]
        return stats[0]

    def SetJacobian(self, mode):
        """uw::Tracker::SetJacobian (uwt_set_jacobian): 0 / "reference" the reference's Jw, 1 / "metric" the 3-D point's coordinates in
        columns 2..5 — every Estimate* call from here on.  Metric is meant to run with handoff "keep" of the seeded calls."""
        self._ctx.set_jacobian(mode)

    def PredictSeeds(self, prev, cur):
        """The constant-velocity motion model in keyframe coordinates (uwt_predict_seeds): prev = the poses keyframe -> frame p - 1,
        cur = keyframe -> frame p, [n, 7] each; returns the seeds (cur * prev^-1) * cur for keyframe -> frame p + 1."""
        return self._ctx.predict_seeds(prev, cur)

    def FastEstimatePose(self, _previous_frame, _current_frame):
        """include/Tracker.h:124 — the vectorised prototype's schedule (levels PYRAMID_LEVELS-1 .. 0, <= 50 iterations,
        gain 50; src/Tracker.cpp:877-885, 1082) over EstimatePose's per-point terms.  The reference body is broken
        (residual ignores the warp :933-944, Jw1 column 0 zeroed :986) and is not reproduced."""
        a, b = self._bind(_previous_frame), self._bind(_current_frame)
        if not _previous_frame.obtained_gradients_:
            raise RuntimeError("ApplyGradient(previous_frame) must run before FastEstimatePose (or its slot was reused since)")
        keys = ("first_level", "last_level", "max_iters", "gain", "epsilon", "z_factor", "angle_factor", "early_exit", "handoff_scale_t")
        saved = {k: getattr(self._ctx.params, k) for k in keys}
        self._ctx.update_params(first_level=self._ctx.params.n_levels - 1, last_level=0, max_iters=50, gain=50.0, epsilon=0.001,
                                z_factor=1.0, angle_factor=1.0, early_exit=1, handoff_scale_t=0)
        try:
            poses, stats = self._ctx.estimate_pose_batch([a], [b], raise_on_pair_failure=True)
        finally:
            self._ctx.update_params(**saved)
        _previous_frame.rigid_transformation_ = poses[0]
        return stats[0]

    def ObtainCandidatePoints(self, _frame, gradient_threshold=20.0):
        """src/Tracker.cpp:1314-1398 (GRADIENT_THRESHOLD, src/Options.cpp:27)."""
        slot = self._bind(_frame)
        for l in range(self._ctx.params.n_levels):
            _frame.candidatePoints_[l] = self._ctx.obtain_candidate_points(slot, l, gradient_threshold)[0]
        _frame.obtained_candidatePoints_ = True

    def ObtainPatchesPoints(self, _previous_frame):
        """src/Tracker.cpp:1178-1257."""
        slot = self._bind(_previous_frame)
        _previous_frame.candidatePoints_[0] = self._ctx.obtain_patch_points(slot, _previous_frame.keypoints_)[0]
        _previous_frame.obtained_candidatePoints_ = True

    def AddPatchPointsFeatures(self, candidatePoints, lvl, patch_size=5):
        """src/Tracker.cpp:599-629 (include/Tracker.h:126): the N x 4 table plus the patch cells around every point."""
        return self._ctx.add_patch_points(lvl, candidatePoints, patch_size)[0]

    def Mat2SE3(self, _input):
        """src/Tracker.cpp:1596-1605 (include/Tracker.h:178): 6 x 1 [w1 w2 w3 x1 x2 x3] -> SE3(SO3::exp(w), x) — the
        translation is taken as it is, not through V(w).  Returns qx qy qz qw tx ty tz."""
        v = np.asarray(_input, np.float32).reshape(6)
        pose = self._ctx.se3_exp(np.array([0, 0, 0, v[0], v[1], v[2]], np.float32))   # rotation part of exp; V(w) * 0 = 0
        pose[4:] = v[3:]
        return pose

    def EstimatePoseFeatures(self, _previous_frame, _current_frame):
        """src/Tracker.cpp:632-872 — the reference's live variant (constants :634-640, :834, :856)."""
        a, b = self._bind(_previous_frame), self._bind(_current_frame)
        if not _previous_frame.obtained_gradients_:
            raise RuntimeError("ApplyGradient(previous_frame) must run before EstimatePoseFeatures (or its slot was reused since)")
        saved = {k: getattr(self._ctx.params, k) for k in ("first_level", "last_level", "max_iters", "gain", "z_factor",
                                                            "angle_factor", "handoff_scale_t", "early_exit")}
        # (z_factor 0.002 compensates the pixel coordinate in the reference's column 2: 1 under the metric Jacobian, as in the batched call)
        zf = 1.0 if self._ctx.get_jacobian() == capi.JACOBIAN_METRIC else 0.002
        self._ctx.update_params(first_level=0, last_level=0, max_iters=10, gain=1.0, z_factor=zf, angle_factor=1.0,
                                handoff_scale_t=1, early_exit=1)
        try:
            pose, st = self._ctx.estimate_pose_points(a, b, {0: _previous_frame.candidatePoints_[0]})
        finally:
            self._ctx.update_params(**saved)
        _previous_frame.rigid_transformation_ = pose
        return st

    def EstimatePoseFeaturesBatch(self, _pairs, weights=None, sampler=None, seeds=None, handoff=None):
        """System::Tracking's live call (src/System.cpp:214-219) for a list of (previous, current) frame pairs in one call
        (uwt_estimate_pose_features_batch, as uw::Tracker::EstimatePoseFeaturesBatch): each previous frame's keypoints_ go in,
        its rigid_transformation_ comes out.  The reference's constants are the call's own; the tracker's params are not touched.
        weights (0 identity, 1 Tukey, 2 Huber) / sampler (0 round(), 1 bilinear), either given: the call's own options
        (uwt_estimate_pose_features_batch_opt).  seeds ([P, 7]) / handoff, either given: the pairs' start poses
        (uwt_estimate_pose_features_batch_seeded).  Returns the per-pair stats."""
        slots = [(self._bind(a), self._bind(b)) for a, b in _pairs]
        for (a, b), (sa, sb) in zip(_pairs, slots):   # binding a later pair's frame may have taken an earlier frame's slot
            if a._slot != sa or b._slot != sb:
                raise RuntimeError("EstimatePoseFeaturesBatch: more frames than slots (max_frames)")
            if not a.obtained_gradients_:
                raise RuntimeError("ApplyGradient(previous_frame) must run before EstimatePoseFeaturesBatch (or its slot was reused since)")
        if seeds is None and handoff is None:
            poses, stats = self._ctx.estimate_pose_features_batch([s[0] for s in slots], [s[1] for s in slots],
                                                                  [a.keypoints_ for a, _ in _pairs], weights=weights, sampler=sampler)
        else:
            poses, stats = self._ctx.estimate_pose_features_batch_seeded([s[0] for s in slots], [s[1] for s in slots],
                                                                         [a.keypoints_ for a, _ in _pairs], seeds, handoff,
                                                                         weights=weights, sampler=sampler)
        for (a, _), pose in zip(_pairs, poses):
            a.rigid_transformation_ = pose.copy()
        return stats

    def EstimatePoseCandidatesBatch(self, _pairs, gradient_threshold=20.0, weights=None, sampler=None, seeds=None, handoff=None):
        """Semi-dense tracking for a list of (previous, current) frame pairs in one call (uwt_estimate_pose_candidates_batch, as
        uw::Tracker::EstimatePoseCandidatesBatch): ObtainCandidatePoints(previous) on the iterated levels, then EstimatePose over
        those tables under the tracker's params; each previous frame's rigid_transformation_ comes out.  weights / sampler, either
        given: the call's own options (uwt_estimate_pose_candidates_batch_opt).  seeds ([P, 7]) / handoff, either given: the pairs'
        start poses (uwt_estimate_pose_candidates_batch_seeded; the weights and the sampler are then the call's, identity and round()
        unless given).  Returns the per-pair stats."""
        slots = [(self._bind(a), self._bind(b)) for a, b in _pairs]
        for (a, b), (sa, sb) in zip(_pairs, slots):   # binding a later pair's frame may have taken an earlier frame's slot
            if a._slot != sa or b._slot != sb:
                raise RuntimeError("EstimatePoseCandidatesBatch: more frames than slots (max_frames)")
            if not a.obtained_gradients_:
                raise RuntimeError("ApplyGradient(previous_frame) must run before EstimatePoseCandidatesBatch (or its slot was reused since)")
        if seeds is None and handoff is None:
            poses, stats = self._ctx.estimate_pose_candidates_batch([s[0] for s in slots], [s[1] for s in slots], gradient_threshold,
                                                                    weights=weights, sampler=sampler)
        else:
            poses, stats = self._ctx.estimate_pose_candidates_batch_seeded([s[0] for s in slots], [s[1] for s in slots], seeds, handoff,
                                                                           gradient_threshold, weights=weights, sampler=sampler)
        for (a, _), pose in zip(_pairs, poses):
            a.rigid_transformation_ = pose.copy()
        return stats

    def ObtainGradientXY(self, _inputImage):
        """include/Tracker.h:197 — (gradientX, gradientY) = 3 x Scharr of a u8 image, CV_16S (src/Tracker.cpp:1133-1134)."""
        return self._ctx.scharr3(_inputImage)

    def MedianMat(self, _input):
        """include/Tracker.h:206, src/Tracker.cpp:1571-1594."""
        return self._ctx.robust_weights(_input, kind=0, want_weights=False)[1]

    def MedianAbsoluteDeviation(self, x):
        """include/Tracker.h:216, src/Tracker.cpp:1607-1619."""
        return self._ctx.robust_weights(x, kind=0, want_weights=False)[2]

    def IdentityWeights(self, _num_residuals):
        """include/Tracker.h:224, src/Tracker.cpp:1621-1624."""
        return self._ctx.robust_weights(np.zeros(int(_num_residuals), np.float32), kind=0)[0]

    def TukeyFunctionWeights(self, _residuals):
        """include/Tracker.h:235, src/Tracker.cpp:1626-1654."""
        return self._ctx.robust_weights(_residuals, kind=1)[0]

    def GetFrameData(self, _frame, lvl, plane):
        return self._ctx.get_plane(self._bind(_frame), lvl, plane)

    def _find_plane(self, _image):
        """(slot, level) of an image the device holds: a Frame (its level 0), a (Frame, lvl) pair, or pixels — the level is the one of
        that size, the slot the resident frame whose plane at that level (GetFrameData) has these pixels.  Pixels of level 0's size
        that no resident frame has are uploaded as a frame of their own (it takes the least-recently-used slot); pixels of a coarser
        level's size that are nowhere on the device cannot be placed: the device builds levels 1.. from level 0."""
        if isinstance(_image, Frame):
            return self._bind(_image), 0
        if isinstance(_image, tuple):
            return self._bind(_image[0]), int(_image[1])
        img = np.ascontiguousarray(_image, np.uint8)
        n = self._ctx.params.n_levels
        sizes = [(L.img_h, L.img_w) for L in (self._ctx.level_info(l) for l in range(n))]
        if img.shape not in sizes:
            raise ValueError("the image has the size of no pyramid level")
        lvl = sizes.index(img.shape)
        for slot, f in enumerate(self._owner):
            if f is None:
                continue
            plane = f.images_[0] if lvl == 0 else self._ctx.get_plane(slot, lvl, capi.PLANE_IMAGE)
            if plane is img or np.array_equal(plane, img):
                return self._bind(f), lvl
        if lvl != 0:
            raise ValueError("an image of a coarser level's size that is no resident plane cannot be placed on the device")
        self._scratch_frame = Frame(img)
        return self._bind(self._scratch_frame), 0

    def ObtainImageTransformed(self, _originalImage, _candidatePoints, _warpedPoints, _outputImage):
        """include/Tracker.h:188, src/Tracker.cpp:1473-1525: _outputImage[round(warped)] = _originalImage[(int)point] for every row
        in order, the last row on a pixel winning; _outputImage is written in place (pixels no row lands on keep their content) and
        validPixel returned.  _originalImage: see _find_plane."""
        slot, lvl = self._find_plane(_originalImage)
        out, valid = self._ctx.obtain_image_transformed(slot, lvl, _candidatePoints, _warpedPoints, _outputImage)
        _outputImage[...] = out
        return valid

    def DebugShowWarpedPerspective(self, _image1, _image2, _imageWarped, _lvl):
        """include/Tracker.h:257, src/Tracker.cpp:1694-1737: the four-panel image [image1 | image2] over [blend(warped, image2) |
        blend(image1, image2)], returned instead of shown (imshow / waitKey and the window's resize loop are the caller's).  _lvl is
        the reference's argument; the level is the one of the images' size.  _image1, _image2: see _find_plane."""
        a, la = self._find_plane(_image1)
        b, lb = self._find_plane(_image2)
        if la != lb or self._owner[a] is None or self._owner[a]._slot != a:
            raise RuntimeError("DebugShowWarpedPerspective: images of two levels, or more frames than slots (max_frames)")
        return self._ctx.warp_mosaic(a, b, la, _imageWarped)

    def WarpedImageBatch(self, pairs, poses, lvl=0):
        """ObtainAllPoints -> WarpFunction -> ObtainImageTransformed for a list of (previous, current) frame pairs under `poses`
        ([P, 7]) in one call (uwt_warp_image_batch): returns (warped [P, h, w], valid [P, h, w], quality [P] capi.WARP_QUALITY)."""
        slots = [(self._bind(a), self._bind(b)) for a, b in pairs]
        for (a, b), (sa, sb) in zip(pairs, slots):   # binding a later pair's frame may have taken an earlier frame's slot
            if a._slot != sa or b._slot != sb:
                raise RuntimeError("WarpedImageBatch: more frames than slots (max_frames)")
        r = self._ctx.warp_image_batch([s[0] for s in slots], [s[1] for s in slots], poses, lvl=lvl, absdiff=False)
        return r["warped"], r["valid"], r["quality"]

    def PointCloudBatch(self, frames, traj, params=None):
        """Visualizer::AddPointCloudFromRGBD for a list of frames under the accumulated poses `traj` ([F, 7]) in one call
        (uwt_point_cloud_batch): returns (points capi.CLOUD_POINT in frame order and, inside a frame, in row order; info [F]
        capi.CLOUD_INFO; the call's record).  params None: the reference's call (the dense level-0 table, every 100th row)."""
        params = capi.default_cloud_params() if params is None else params
        slots = [self._bind(f) for f in frames]
        for f, s in zip(frames, slots):   # binding a later frame may have taken an earlier frame's slot
            if f._slot != s:
                raise RuntimeError("PointCloudBatch: more frames than slots (max_frames)")
            if params.source == 1 and not f.obtained_gradients_:
                raise RuntimeError("PointCloudBatch: the candidate source needs ApplyGradient (or the frame's slot was reused since)")
        r = self._ctx.point_cloud_batch(slots, traj, params)
        return r["points"], r["info"], r["call"]

    def SweepDepth(self, keyframe, views, poses, codes, params=None):
        """EXTENSION (no reference counterpart): the keyframe's depth codes from the 1..4 frames `views` tracked against it and their
        poses ([n_views, 7], X_view = T X_keyframe — what the tracking calls return), one job of uwt_sweep_depth_batch.  codes: the u16
        hypotheses (capi.sweep_hypotheses).  Returns (depth u16, cost u16, outcome u8 — the level's img_h x img_w — and the job's
        capi.SWEEP_INFO record)."""
        frames = [keyframe] + list(views)
        codes = np.ascontiguousarray(codes, np.uint16).reshape(-1)
        if params is None:
            params = capi.default_sweep_params(n_views=len(views), n_hyp=codes.size)
        slots = [self._bind(f) for f in frames]
        for f, s in zip(frames, slots):   # binding a later frame may have taken an earlier frame's slot
            if f._slot != s:
                raise RuntimeError("SweepDepth: more frames than slots (max_frames)")
        if params.source == 1 and not keyframe.obtained_gradients_:
            raise RuntimeError("SweepDepth: the candidate source needs ApplyGradient on the keyframe (or its slot was reused since)")
        r = self._ctx.sweep_depth([slots[0]], [slots[1:]], poses, codes, params)
        return r["depth"][0], r["cost"][0], r["outcome"][0], r["info"][0]


class Map:
    """include/Map.h — Map::AddPointCloudFromRGBD (src/Map.cpp:33-45): recent_cloud_points_ is the x y z columns of the frame's
    level-0 candidatePoints_; PointCloudBatch: the tracker's batch call."""

    def __init__(self, tracker=None):
        self._tracker = tracker
        self.recent_cloud_points_ = np.zeros((0, 3), np.float32)

    def AddPointCloudFromRGBD(self, frame):
        if 0 not in frame.candidatePoints_:   # the dense ObtainAllPoints keeps no table
            raise RuntimeError("Map.AddPointCloudFromRGBD: the frame has no level-0 candidatePoints_")
        self.recent_cloud_points_ = np.asarray(frame.candidatePoints_[0], np.float32).reshape(-1, 4)[:, :3]   # a view, N x 3

    def PointCloudBatch(self, frames, traj, params=None):
        return self._tracker.PointCloudBatch(frames, traj, params)


class Visualizer:
    """The map-building part of include/Visualizer.h — Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446) on the device:
    every 100th row of the frame's level-0 table (its candidatePoints_[0] when a sparse producer ran, else ObtainAllPoints' dense
    table of the bound frame), unprojected and offset by previous_pose's translation, appended to point_cloud_.  previous_pose is
    the accumulation UpdateMessages keeps (accumulate_trajectory with t_scale 40, reference_axes False); the tags count the calls."""

    def __init__(self, tracker):
        self._tracker = tracker
        self.point_cloud_ = np.zeros(0, capi.CLOUD_POINT)
        self.previous_pose_ = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
        self._n_calls = 0

    def AddPointCloudFromRGBD(self, frame, previous_pose):
        self.previous_pose_ = np.array(previous_pose, np.float32).reshape(7)
        if 0 in frame.candidatePoints_:
            rec = self._tracker._ctx.point_cloud_points(self._tracker._bind(frame), frame.candidatePoints_[0], self.previous_pose_)[0]
        else:
            rec = self._tracker.PointCloudBatch([frame], self.previous_pose_[None])[0]
        rec = rec.copy()
        rec["tag"] = (rec["tag"] & 255) | np.uint32(self._n_calls << 8)
        self._n_calls += 1
        self.point_cloud_ = np.concatenate([self.point_cloud_, rec])


class RobustMatcher:
    """include/Tracker.h:65-88 — the matching half of RobustMatcher::DetectAndTrackFeatures (src/Tracker.cpp:171-258): knnMatch in
    both directions, ratioTest twice and symmetryTest, on the GPU over the C ABI (uwt_match_descriptors_batch), ransacTest as the
    inlier selection of uwt_ransac_inliers_batch (the contract: include/uwt.h; cv::findFundamentalMat itself draws from OpenCV's RNG
    and is not pinned); getGoodKeypoints and the assignment of :247-254 on the host.  Detection and description with
    cuda::SURF_CUDA (:186-206) are uwt_surf_detect_describe_batch / uwt_surf_describe_batch, SURF under the contract of include/uwt.h:
    DetectAndTrackFeatures(previous, current, usekeypoints) is the reference's whole method.  With detector=1, as
    RobustMatcher(int detector) of src/Tracker.cpp:38-46, the same method runs cuda::ORB's branch (:210-223):
    uwt_orb_detect_describe_batch / uwt_orb_describe_batch, ORB under the contract of include/uwt.h, matched under Hamming; the full
    records are kept in Frame.orb_keypoints_.  The forms that take the caller's descriptors stay.  A caller with a RANSAC of their
    own still hands its inlier mask to MatchAndSetKeypoints.
    float32 descriptors are matched under L2 (SURF), uint8 under Hamming (ORB), as createBFMatcher is set up at :199 / :221."""

    def __init__(self, ctx_or_tracker, ratio=0.65, distance=3.0, confidence=0.99, refineF=True, detector=0):
        if detector not in (0, 1):
            raise ValueError("RobustMatcher: detector is 0 (SURF) or 1 (ORB)")
        self._src = ctx_or_tracker
        self.detector_ = int(detector)           # src/Tracker.cpp:38-46: 0 SURF, 1 ORB
        self.ratio_ = float(np.float32(ratio))   # include/Tracker.h:80
        self.distance_ = float(distance)         # include/Tracker.h:82
        self.confidence_ = float(confidence)     # include/Tracker.h:83
        self.refineF_ = bool(refineF)            # include/Tracker.h:81; a documented no-op: the refit's result is discarded by the
                                                 # reference (src/Tracker.cpp:124, 141-166), so there is nothing to compute
        self.max_hypotheses_ = 1000              # no reference member: the budget of the selection (uwt_ransac_params)
        self.seed_ = 0
        self.hessian_threshold_ = 100.0          # cuda::SURF_CUDA's defaults (`cuda::SURF_CUDA surf;`, src/Tracker.cpp:188)
        self.n_octaves_, self.n_octave_layers_, self.upright_ = 4, 2, False
        self.n_features_, self.n_levels_ = 500, 8   # cuda::ORB::create()'s defaults (src/Tracker.cpp:212)
        self.edge_threshold_, self.fast_threshold_ = 31, 20
        self.orb_pattern_ = None                 # None: the library's default pattern; else int8 [256, 4] (uwt_orb_set_pattern)
        self._pattern_sent = None

    @property
    def _ctx(self):
        ctx = getattr(self._src, "_ctx", self._src)   # a Tracker (after InitializePyramid) or a capi.Context
        if ctx is None:
            raise RuntimeError("RobustMatcher: the Tracker has no context yet (InitializePyramid first)")
        return ctx

    def MatchDescriptors(self, desc_prev, desc_cur):
        """symMatches of one pair (src/Tracker.cpp:202-236): a capi.MATCH record array (query_idx into desc_prev, train_idx into
        desc_cur, distance), ascending query_idx."""
        return self.MatchDescriptorsBatch([(desc_prev, desc_cur)])[0]

    def MatchDescriptorsBatch(self, pairs):
        """The same for a list of (desc_prev, desc_cur) pairs in one call."""
        return self._ctx.match_descriptors_batch(pairs, ratio=self.ratio_)

    def _ransac_params(self):
        return capi.default_ransac_params(distance=self.distance_, confidence=self.confidence_, max_hypotheses=self.max_hypotheses_,
                                          seed=self.seed_)

    def ransacTest(self, matches, keypoints1, keypoints2, outMatches=None):
        """src/Tracker.cpp:105-169: the matches that survive the epipolar test, in their order (goodMatches).  outMatches: an
        optional list that receives them, as the reference's output argument.  Returns (outMatches, inlier mask, info): what the
        reference returns, the fundamental matrix, is an empty Mat there (the local of :124 shadows it); info["F"] has the one the
        selection chose."""
        mask, good, info = self.ransacTestBatch([(matches, keypoints1, keypoints2)])[0]
        if outMatches is not None:
            outMatches[:] = list(good)
        return good, mask, info

    def ransacTestBatch(self, pairs):
        """The same for a list of (matches, keypoints1, keypoints2) in one call."""
        return self._ctx.ransac_inliers_batch(pairs, params=self._ransac_params())

    def DetectAndTrackFeatures(self, _previous_frame, _current_frame, *args, usekeypoints=None):
        """src/Tracker.cpp:171-258.  DetectAndTrackFeatures(previous, current, usekeypoints), the reference's signature: SURF on
        both frames on the device (the previous frame is described at the key points it kept when usekeypoints is set and it has
        some, :192-195; the current one is detected), symmetric matches -> ransacTest -> getGoodKeypoints -> keypoints_,
        surf_keypoints_ and n_matches_ of both frames.  DetectAndTrackFeatures(previous, current, desc_prev, desc_cur, keypoints):
        the same from the matcher on, with the caller's detector output.  Returns the matches kept."""
        if len(args) >= 3:
            return self._track_descriptors(_previous_frame, _current_frame, *args[:3])
        if len(args) == 2:
            raise TypeError("DetectAndTrackFeatures(previous, current, usekeypoints) or (previous, current, desc_prev, desc_cur, keypoints)")
        usekeypoints = bool(args[0]) if args else bool(usekeypoints)
        tracker = self._src
        if not hasattr(tracker, "_bind"):
            raise RuntimeError("DetectAndTrackFeatures(previous, current, usekeypoints) needs a RobustMatcher built over a Tracker")
        a, b = tracker._bind(_previous_frame), tracker._bind(_current_frame)
        if _previous_frame._slot != a:
            raise RuntimeError("DetectAndTrackFeatures: more frames than slots (max_frames)")
        build, detect, describe, kept = self._DETECTORS[self.detector_]
        params = build(self)
        ctx = self._ctx
        if self.detector_ == 1 and self.orb_pattern_ is not self._pattern_sent:   # (the context keeps a pattern until it is given another)
            ctx.orb_set_pattern(self.orb_pattern_)
            self._pattern_sent = self.orb_pattern_
        if usekeypoints and len(getattr(_previous_frame, kept)):
            kp0, d0 = getattr(ctx, describe)([a], [getattr(_previous_frame, kept)], params=params)[0]
            kp1, d1 = getattr(ctx, detect)([b], params=params)[0]
        else:
            (kp0, d0), (kp1, d1) = getattr(ctx, detect)([a, b], params=params)
        xy = (np.stack([kp0["x"], kp0["y"]], 1), np.stack([kp1["x"], kp1["y"]], 1))
        good = self._track_descriptors(_previous_frame, _current_frame, d0, d1, xy)   # (float32 rows: L2; uint8 rows: Hamming)
        setattr(_previous_frame, kept, kp0[good["query_idx"]])
        setattr(_current_frame, kept, kp1[good["train_idx"]])
        return good

    # per detector (src/Tracker.cpp:186-206 SURF, :210-223 ORB): the params builder, the context's detect and describe-at-given
    # methods, and the frame attribute that holds the records kept; the norm follows from the descriptors' dtype (MatchDescriptors)
    _DETECTORS = {
        0: (lambda self: capi.default_surf_params(hessian_threshold=self.hessian_threshold_, n_octaves=self.n_octaves_,
                                                  n_octave_layers=self.n_octave_layers_, upright=int(self.upright_)),
            "surf_detect_describe_batch", "surf_describe_batch", "surf_keypoints_"),
        1: (lambda self: capi.default_orb_params(n_features=self.n_features_, n_levels=self.n_levels_, edge_threshold=self.edge_threshold_,
                                                 fast_threshold=self.fast_threshold_, upright=int(self.upright_)),
            "orb_detect_describe_batch", "orb_describe_batch", "orb_keypoints_"),
    }

    def _track_descriptors(self, _previous_frame, _current_frame, desc_prev, desc_cur, keypoints):
        matches = self.MatchDescriptors(desc_prev, desc_cur)
        good, _, _ = self.ransacTest(matches, keypoints[0], keypoints[1])
        return self.SetKeypoints(_previous_frame, _current_frame, good, keypoints)

    def SetKeypoints(self, _previous_frame, _current_frame, goodMatches, keypoints):
        """getGoodKeypoints and the assignment of src/Tracker.cpp:241-254"""
        good = self.getGoodKeypoints(goodMatches, keypoints)
        _previous_frame.n_matches_ = _current_frame.n_matches_ = len(goodMatches)
        _previous_frame.keypoints_, _current_frame.keypoints_ = good
        return goodMatches

    @staticmethod
    def getGoodKeypoints(goodMatches, keypoints):
        """src/Tracker.cpp:260-270: keypoints = (previous [n, 2], current [m, 2]); returns the matched rows of each, in match order."""
        k0, k1 = (np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints)
        return k0[goodMatches["query_idx"]], k1[goodMatches["train_idx"]]

    def MatchAndSetKeypoints(self, _previous_frame, _current_frame, desc_prev, desc_cur, keypoints, inlier_mask=None):
        """DetectAndTrackFeatures from the matcher on (src/Tracker.cpp:224-254) with the caller's detector output: symmetric
        matches, the caller's optional RANSAC inlier mask over them (or a callable matches -> mask), getGoodKeypoints, then
        keypoints_ and n_matches_ of both frames (:247-254).  Tracker::EstimatePoseFeatures / the batched live call can follow
        directly.  n_matches_ feeds the caller's `n_matches_ < 110` rule (src/System.cpp:208), which stays with the caller.
        Returns the matches kept."""
        matches = self.MatchDescriptors(desc_prev, desc_cur)
        if callable(inlier_mask):
            inlier_mask = inlier_mask(matches)
        if inlier_mask is not None:
            matches = matches[np.asarray(inlier_mask, bool)]
        good = self.getGoodKeypoints(matches, keypoints)
        _previous_frame.n_matches_ = _current_frame.n_matches_ = len(matches)
        _previous_frame.keypoints_, _current_frame.keypoints_ = good
        return matches


def Tracking(tracker, robust_matcher, previous_frame, current_frame):
    """System::Tracking() (src/System.cpp:193-223), the live loop's body for one pair, every call on the device: ApplyGradient of both
    frames, DetectAndTrackFeatures(previous, current, usekeypoints) with the `n_matches_ < 110` rule of :208, ObtainPatchesPoints,
    EstimatePoseFeatures -> previous_frame.rigid_transformation_.  Returns the alignment's stats."""
    usekeypoints = True
    if not previous_frame.obtained_gradients_:
        tracker.ApplyGradient(previous_frame)
    tracker.ApplyGradient(current_frame)
    if previous_frame.n_matches_ < 110:
        usekeypoints = False
    robust_matcher.DetectAndTrackFeatures(previous_frame, current_frame, usekeypoints)
    tracker.ObtainPatchesPoints(previous_frame)
    return tracker.EstimatePoseFeatures(previous_frame, current_frame)


def TrackingBatch(tracker, robust_matcher, pairs, cap=2048, seeds=None):
    """System::Tracking() for a list of (previous_frame, current_frame) pairs through the device-resident call
    (uwt_tracking_batch, or uwt_tracking_orb_batch for RobustMatcher(detector=1)): the detector, the matcher, ransacTest,
    getGoodKeypoints and the live alignment run as one chain on the device, and keypoints_, surf_keypoints_ (orb_keypoints_ with ORB),
    n_matches_ of both frames and previous_frame.rigid_transformation_ end up exactly as the Tracking loop over the same list with the
    same matcher leaves them.  Pairs that share no frame go into one call; a pair that names a frame an earlier
    pair of the list has written (the next pair of a sequence) waits for that pair's results, as it does in the loop.  Returns
    the per-pair stats; a pair without a good match has ERR_NO_VALID_POINTS there and its frames' lists empty.
    seeds ([len(pairs), 7]): the pairs' start poses for the live alignment (uwt_tracking_batch_seeded / uwt_tracking_orb_batch_seeded);
    the front end is untouched, and a pair it fails keeps the identity."""
    ctx = tracker._ctx
    rm = robust_matcher
    build, _, _, kept = rm._DETECTORS[rm.detector_]
    detector_params = build(rm)
    common = dict(ransac=dict(distance=rm.distance_, confidence=rm.confidence_, max_hypotheses=rm.max_hypotheses_, seed=rm.seed_),
                  ratio=rm.ratio_, min_matches=110)
    fields = {k: getattr(detector_params, k) for k, _ in detector_params._fields_}
    if rm.detector_ == 1:
        params, call = capi.default_tracking_orb_params(orb=fields, **common), ctx.tracking_orb_batch
        seeded_call = ctx.tracking_orb_batch_seeded
        if rm.orb_pattern_ is not rm._pattern_sent:   # as DetectAndTrackFeatures: the context keeps a pattern until it is given another
            ctx.orb_set_pattern(rm.orb_pattern_)
            rm._pattern_sent = rm.orb_pattern_
    else:
        params, call = capi.default_tracking_params(surf=fields, **common), ctx.tracking_batch
        seeded_call = ctx.tracking_batch_seeded
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, np.float32).reshape(len(pairs), 7)
    stats, i = [], 0
    while i < len(pairs):
        run, seen = [], set()
        while i < len(pairs) and len(run) < ctx.params.max_pairs and not ({id(pairs[i][0]), id(pairs[i][1])} & seen):
            run.append(pairs[i])
            seen |= {id(pairs[i][0]), id(pairs[i][1])}
            i += 1
        for a, b in run:
            if not a.obtained_gradients_:
                tracker.ApplyGradient(a)
            tracker.ApplyGradient(b)
        slots = [(tracker._bind(a), tracker._bind(b)) for a, b in run]
        for (a, b), (sa, sb) in zip(run, slots):   # binding a later pair's frame may have taken an earlier frame's slot
            if a._slot != sa or b._slot != sb or not (a.obtained_gradients_ and b.obtained_gradients_):
                raise RuntimeError("TrackingBatch: more frames than slots (max_frames)")
        if seeds is None:
            r = call([s[0] for s in slots], [s[1] for s in slots], prev=[getattr(a, kept) for a, _ in run], params=params, cap=cap)
        else:
            r = seeded_call([s[0] for s in slots], [s[1] for s in slots], prev=[getattr(a, kept) for a, _ in run], params=params, cap=cap,
                            seeds=seeds[i - len(run):i])
        for k, (a, b) in enumerate(run):
            kp0, kp1 = r["kept_prev"][k], r["kept_cur"][k]
            a.n_matches_ = b.n_matches_ = len(kp0)
            a.keypoints_, b.keypoints_ = np.stack([kp0["x"], kp0["y"]], 1), np.stack([kp1["x"], kp1["y"]], 1)
            setattr(a, kept, kp0)
            setattr(b, kept, kp1)
            a.rigid_transformation_ = r["poses"][k].copy()
            st = r["stats"][k]
            stats.append(dict(status=int(st["status"]), iterations=int(st["iterations"]), n_valid=int(st["n_valid"]), error=float(st["error"])))
    return stats


class LS:
    """include/LeastSquares.h:26-50 over the GPU reduction: rows are buffered by update() / updateSSE() and folded by
    finish*() — scalar rows through uwt_ls_accumulate, 4-wide rows through uwt_ls_accumulate_sse (the two forms associate
    their products differently, src/LeastSquares.cpp:151-153 vs :205), the two added as finishNoDivide adds the lane sums
    onto A, b, error (:39-139)."""

    _default_ctx = None                         # the context `LS()` folds on: LS.bind(ctx), else a small one of its own

    @classmethod
    def bind(cls, ctx):
        """The context a default-constructed LS uses (the reference writes `LS ls;`, src/Tracker.cpp:537)."""
        cls._default_ctx = ctx

    def __init__(self, ctx=None, count_quirk=True):
        self._ctx_arg = ctx
        self.count_quirk = count_quirk          # "num_constraints += 6" per updateSSE call (src/LeastSquares.cpp:201)
        self.initialize(0)

    @property
    def _ctx(self):
        if self._ctx_arg is not None:
            return self._ctx_arg
        if LS._default_ctx is not None and not LS._default_ctx._h:
            LS._default_ctx = None              # the context it was bound to has been closed
        if LS._default_ctx is None:             # nothing bound: a minimal context just for the reductions
            LS._default_ctx = capi.Context(capi.default_params(64, 48, 64.0, 64.0, 31.5, 23.5, n_levels=1, first_level=0,
                                                               last_level=0, max_frames=2, max_pairs=1))
        return LS._default_ctx

    def initialize(self, max_num_constraints):
        self._J, self._r, self._w = [], [], []
        self._J4, self._r4, self._w4 = [], [], []
        self.A = np.zeros((6, 6), np.float32)
        self.b = np.zeros(6, np.float32)
        self.error = 0.0
        self.num_constraints = 0

    def update(self, J, res, weight):
        self._J.append(np.asarray(J, np.float32).reshape(6))
        self._r.append(res)
        self._w.append(weight)

    def updateSSE(self, J1, J2, J3, J4, J5, J6, res, weight):
        """Four points at once; J1..J6 hold Jacobian component k of the four points (include/LeastSquares.h:42-43)."""
        Jc = np.stack([np.asarray(x, np.float32).reshape(4) for x in (J1, J2, J3, J4, J5, J6)])   # 6 x 4
        self._J4.append(Jc.T.copy())                                                              # 4 rows of 6
        self._r4.append(np.asarray(res, np.float32).reshape(4))
        self._w4.append(np.asarray(weight, np.float32).reshape(4))

    def _fold(self, divide):
        A = np.zeros((6, 6), np.float32); b = np.zeros(6, np.float32); err = np.float32(0); n = 0
        if self._r:
            A1, b1, e1, n1 = self._ctx.ls_accumulate(np.stack(self._J), np.array(self._r, np.float32), np.array(self._w, np.float32), False)
            A, b, err, n = A + A1, b + b1, np.float32(err + np.float32(e1)), n + n1
        if self._r4:
            A2, b2, e2, n2 = self._ctx.ls_accumulate_sse(np.concatenate(self._J4), np.concatenate(self._r4), np.concatenate(self._w4),
                                                         False, self.count_quirk)
            A, b, err, n = A + A2, b + b2, np.float32(err + np.float32(e2)), n + n2
        if divide:   # unconditional, as LS::finish (src/LeastSquares.cpp:141-146) and uw::LS::finish: an empty system gives NaN
            fn = np.float32(n)
            with np.errstate(divide="ignore", invalid="ignore"):
                A, b, err = A / fn, b / fn, np.float32(np.float32(err) / fn)
        self.A, self.b, self.error, self.num_constraints = A.astype(np.float32), b.astype(np.float32), float(err), n

    def finishNoDivide(self):
        self._fold(False)

    def finish(self):
        self._fold(True)
