"""TEST HARNESS: model-based random call sequences over the surface the lifecycle harness does not know -- alpha mode, index output,
error statistics and reduce_quality, frame sequences, fixed colours, lossy delta frames -- on ONE long-lived processor
(tests/test_session_model.py on the CPU, tools/fuzz_session.py and tests/test_gpu_session.py on the device).  A sibling of
tests/lifecycle_harness.py, from which it takes KgEnv's memory interface, Mismatch, the guard bytes and the generate / Runner /
replay / run_sequence shape with plain-tuple ops and a printed replay(...) line on failure.

Every call is a pure function of (pixels, switches as they were when the call -- or the object the call belongs to -- started), so
a stateless model built from tests/oracle_lib.py, alpha_ref, diffuse_ref, fixed_ref, error_ref, sequence_ref and hold_ref predicts
every byte.  What the model tracks is what the ABI defines as state: the three switches; the cutoff each added frame was compacted
under; cutoff, k, centroids, mode and format an open output was begun with; canvas and held source of every open output and of
every caller-owned buffer pair; the running combination of the caller's error record; each Lloyd object's n_fixed.  One sequence
uses one processor, two Lloyd objects, two Sequence objects and two caller-owned canvas pairs, closed and re-created in each
other's blocks.

Surface 2 (generate(..., surface=2), seeds of its own; the lists of surface 1 are pinned by hash) adds, on the same Sequence
objects, switches and blocks: outputs with per-frame palettes (local_ref: cold frames as reduce_indexed, warm frames from the last
frame's centroids on the working image of the cutoff read at the call, shown and held source carried in the model, every coded frame
since the begin replayed after every frame; a call refused before any work is enqueued leaves a warm output warm, a frame that fails
in its palette step makes the next one cold); colour-keyed canvases of the caller's at element offsets that pick the vector or the
per-pixel route, a new palette with repeated entries and a zero word per frame; the index-map optimisation (index_ref): two usage
records and the bad-pixel count, which COMBINE across bands, images and the frames of a sequence, two plan slots, remaps at every
width, kmg_index_optimize between the other calls.

Surface 3 (generate(..., surface=3), seeds of its own; the lists of surfaces 1 and 2 are pinned by hash) adds alpha weighting, the
one sticky switch with the most cross-talk: ("weight", 0|1) on the processor between all the calls above -- it moves the cutoff of
a working image to max(t, 1) where the image is MADE (a host call, an add, a local frame, cold or warm), decides whether a loop is
weighted where the loop STARTS (the palette call of a sequence, not its adds), and leaves every output's cutoff, the error record
of reduce_quality and the initialisation alone; find, apply, compare, the canvases, usage, remap never look at it, and neither does
the model there.  ("l_weight", L, 0|1) on a Lloyd object: weighted sums (weight_ref.accumulate on the alpha bytes of the image
given), the same labels; the model tracks WHO holds the object's binding -- nobody, the initialisation (under the forced colour
table), the caller -- because the setter drops the initialisation's and is refused under the caller's ("l_unbind" where the model
cannot rule a caller's binding out).  One more image, the importance map: 53 x 67, every alpha in 1 .. 255.

Surface 4 (generate(..., surface=4), seeds of its own; the lists of surfaces 1 to 3 are pinned by hash) adds the batched calls, on
the same processor, switches, Lloyd and Sequence objects and blocks: ("b_palette", images, k, algo, bound), ("b_reduce", images, k,
algo, mode, bound), ("b_reduce_indexed", images, k, algo, mode, format, bound), ("b_find", images, k, palette seed, mode, format,
bound) on host buffers, ("b_palette_device", images, k) and ("b_apply_device", images, k, centroid seed, shared, mode, format,
offset) on the resident device copies.  `images` is a list of image indices of length 1, 2 or 3 .. 9, in a random order, an image
may appear twice; `bound` is max_resident_bytes: 0, 1 (a sub-batch per image) or the bytes of two neighbours, which cuts after
every second image.  The model stays stateless: what a batched call gives for image i is what the per-image call gives for image i
under the switches as they stand -- palette, reduce, reduce_indexed, find / find_indexed, apply, and init_centroids + run +
get_centroids for the device call.  The reports are predicted from include/kmeans_hip.h alone: sub_batches by the greedy cut over
the resident bytes the header lists (batch_resident, batch_cut: the model's own few lines), fallback 0 (no working image has 2^19
pixels), iterations the largest count, launches the sum over the k-means sub-batches of two images or more of k + 2 + their largest
count (a sub-batch of one image takes the per-image palette step), and for the output step batched + per_image = n with per_image
= n for meld, diffusion, the octree and the forced table strategy.  After every op: every output, palette and out_counts entry,
the guard bytes, the resident sources of a device call; after a refusal that nothing at all was written -- outputs, counts,
reports -- and that status and message are the header's.

  generate(seed, seq)  -> list of plain tuples (deterministic; a dry Model keeps every op legal or a listed refusal)
  Runner(env).run(ops) -> executes them on a backend, checks everything the op could have touched, raises Mismatch
  replay(env, seed, seq, ops) -> the same for a list printed by a failing run

What the generator never emits, because include/kmeans_hip.h leaves it open or because the lifecycle harness owns it:
  - a pixel buffer that changes while a Lloyd object is bound to it (every image stays resident in a buffer of its own and is
    never rewritten), cell shares, partial sums, kmg_lloyd_prepare;
  - a Lloyd pass before the centroids were set, converged_count before an update, set_fixed above k, more seeds than k;
  - a palette step whose working image is empty, other than the listed refusal on a sequence;
  - kmg_dev_compare with an INDEX8 map of k = 256 under a cutoff argument, k = 0, `what` = 0;
  - a frame of another size than the open output's; bands of an apply plan out of order in KMG_MODE_DIFFUSE;
  - the octree (other than its refusal under fixed colours), meld with an index format (other than its refusal), the group layer;
  - delta bands that overlap or leave rows out: the bands of a frame tile it exactly once;
  - (surface 2) a local frame from the 300 x 200 or the 1024 x 1024 image; an RGBA8 or meld local output, INDEX8 with k = 256 (other
    than their refusals); a usage record combined across maps of different k, or read before it was zeroed; a plan from a record
    with indices above k or without a count (other than the refusals); a remap in place at another width than the map's own, a
    remap whose buffers overlap otherwise; kmg_index_optimize with bits below the plan's (other than the refusal) or above the map's
    width; the colour-keyed passes on buffers that overlap; a palette step whose working image is empty other than the frame of a
    local output at the size of the image without a kept pixel;
  - (surface 3) kmg_lloyd_set_weighting where the model cannot tell whose binding the object holds (it unbinds first), a weighted
    pass of more than 2^28 pixels (tests/test_gpu_weight.py), the group layer's refusal (the harness owns no group).
  - (surface 4) a batch with the 1024 x 1024 image; a dither of 128 colours or more on an image of 16384 pixels or more in a
    batched output step (b_reduce_indexed, b_find, b_apply_device: include/kmeans_hip.h leaves whether it joins the launch to a
    measured rule); diffusion of the 300 x 200 image; the octree under a cutoff above 0, on an image above the shrink limit, in
    b_reduce_indexed, or on the noise images (the reference needs seconds for each); a batch with a palette step on an image
    without a kept pixel, under fixed colours or under weighting (other than the refusals); a NULL array or entry, a zero
    dimension, k = 0 or above KMG_MAX_K, an INDEX16 output at an odd address (tests/test_gpu_batch.py and _apply.py own those).
The 1024 x 1024 image enters host calls and kmg_dev_compare only, and only under the forced colour-table strategy.  The images
are this harness's own (make_images here): frames of one size in families, alpha bytes that fill every cutoff class, a frame above
the shrink limit -- lifecycle_harness.make_images has none of these.  Every sequence mixes random ops with short directed passages
(the motif_* functions of generate), so that each way the state could be mishandled is exercised in every few sequences."""
import collections

import numpy as np

import oracle_lib as O
import alpha_ref
import diffuse_ref
import error_ref
import fixed_ref
import hold_ref
import index_ref
import local_ref
import sequence_ref
import weight_ref
import lifecycle_harness as LH
from lifecycle_harness import Mismatch, GUARD, PATTERN, MAX_ITERATIONS, CHECK_PERIOD, gamut_centroids, make_centroids, sorted_palette

SHRINK = 256
K_CLASSES = ((1, 2), (3, 32), (33, 255), (256, 256), (257, 512))
CUTOFFS = (0, 1, 128, 255)
STRATEGIES = (0, 1, 2)                               # auto, scan, table
IMAGE_KINDS = ("odd", "odd_b", "sprite", "sprite_noisy", "sprite_shift", "few", "flat", "clear", "big", "mega", "row", "row_b", "col",
               "col_b", "map")
ODD, SPRITE, FEW, FLAT, CLEAR, BIG, MEGA, ROW, COL, MAP = 0, 2, 5, 6, 7, 8, 9, 10, 12, 14
FAMILIES = ((0, 1), (2, 3, 4), (10, 11), (12, 13))   # images of one size: the frames of one output
ERR_INVALID = -1
REFUSALS_1 = ("k_below_fixed_palette", "k_below_fixed_reduce", "k_below_fixed_sequence", "octree_fixed", "frame_no_output", "delta_on_rgba8",
              "lossy_on_rgba8", "lossy_without_delta", "index8_full", "meld_indexed", "empty_sequence")
# surface 2: per-frame palettes and the index-map optimisation
REFUSALS_2 = ("shared_frame_on_local", "local_frame_on_shared", "local_frame_no_output", "warm_with_fixed", "local_tolerance_without_delta",
              "local_meld", "local_index8_k256", "plan_indices_above_k", "plan_empty_record", "optimize_bits_too_narrow", "remap_bad_bits")
REFUSALS = REFUSALS_1 + REFUSALS_2
# surface 3: alpha weighting (kmg_processor_set_weighting, kmg_lloyd_set_weighting)
REFUSALS_3 = ("weight_bad_value", "l_weight_bad_value", "octree_weighted", "l_weight_under_caller_binding", "weighted_bind", "weighted_lftu",
              "weighted_accumulate_into", "weighted_no_kept_pixel")
MOTIFS_3 = ("weight_cutoff", "weight_adds", "weight_warm", "weight_binding", "weight_blocks", "weight_fixed", "weight_quality")
LLOYD_IMAGE_OPS = ("l_init", "l_assign_update", "l_iterate", "l_run", "l_lftu", "l_assign", "l_bind")
ERR_UNSUPPORTED = -5
LOCAL_FAMILIES = FAMILIES + ((7,),)                  # a local output needs no added frame: also at the size of the frame without a kept pixel
BITS = (1, 2, 4, 8, 16)
CPAIR_OFFSETS = (0, 4, 1)                            # elements into the allocations: the vector route twice, the per-pixel route
FAILED_KINDS = ("fixed_on_warm", "k_below_fixed", "empty")
TOLERANCES = (0, 40, 4096, 400000)                   # 1/4096 dE76^2: none, under the noise of the still frames, 1 dE, 10 dE
# the fixed lists of set_fixed_colors: none; one colour; three with a duplicate pair; eight with alpha 0, alpha < 255 and a duplicate
FIXED = (None,
         ((200, 30, 40, 255),),
         ((10, 10, 10, 255), (250, 250, 250, 255), (10, 10, 10, 255)),
         ((0, 0, 0, 255), (255, 255, 255, 0), (255, 0, 0, 255), (0, 255, 0, 128), (0, 0, 255, 255), (255, 0, 0, 255), (128, 128, 128, 7),
          (255, 255, 0, 255)))


SURFACE_2_OPS = 120
SURFACE_3_OPS = 70
# surface 4: the batched calls (kmg_palette_batch, kmg_reduce_batch, kmg_reduce_indexed_batch, kmg_find_batch, kmg_dev_palette_batch,
# kmg_dev_apply_batch) on the same processor, switches, objects and blocks
SURFACE_4_OPS = 130
BATCH_OPS = ("b_palette", "b_reduce", "b_reduce_indexed", "b_find", "b_palette_device", "b_apply_device")
REFUSALS_4 = ("batch_fixed", "batch_weighted", "batch_no_kept_pixel", "batch_index8_full", "batch_meld_indexed", "batch_bad_tables", "batch_empty")
MOTIFS_4 = ("batch_shrinking", "batch_device_blocks", "batch_cutoff", "batch_switches", "batch_no_kept_pixel", "batch_beside_objects",
            "batch_octree")
BATCH_POOL = (0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14)     # every image but the one without a kept pixel and the one of 2^20 pixels
BATCH_PALETTE_CALLS = ("b_palette", "b_reduce", "b_reduce_indexed")
# the words of kmg_last_error a refused batch is recognised by
BATCH_NEEDLES = {"batch_fixed": ("fixed colours",), "batch_weighted": ("alpha weighting",), "batch_no_kept_pixel": ("alpha_cutoff",),
                 "batch_index8_full": ("INDEX8",), "batch_meld_indexed": ("no index output",), "batch_bad_tables": ("n_tables",),
                 "batch_empty": ("empty",)}


def k_class(k):
    return next(i for i, (a, b) in enumerate(K_CLASSES) if a <= k <= b)


def n_fixed_of(fid):
    return 0 if FIXED[fid] is None else len(FIXED[fid])


# ---- images ---------------------------------------------------------------------------------------------------------
_images = {}


def make_images(seed, seq):
    """[(kind, (h, w, 4) uint8)] in the order of IMAGE_KINDS.  The smallest shapes at which the kernels branch: an odd-sized noise
    frame and a still copy of it with noise under TOLERANCES[1]; a sprite with soft alpha edges, a noisy still copy and a shifted
    one (pixels that showed a colour turn transparent); a few-colour and a flat image; a frame without a kept pixel; one frame
    above the shrink limit; one of 2^20 pixels; a 1 x N and an N x 1 frame"""
    if (seed, seq) not in _images:
        if len(_images) > 2:
            _images.clear()
        _images[(seed, seq)] = _make_images(seed, seq)
    return _images[(seed, seq)]


def _blobs(rng, w, h):
    c = rng.integers(0, 256, (int(rng.integers(4, 20)), 3))
    a = np.full((h * w, 4), 255, np.uint8)
    a[:, :3] = np.clip(c[rng.integers(0, c.shape[0], h * w)] + rng.normal(0, rng.uniform(3, 20), (h * w, 3)), 0, 255).astype(np.uint8)
    return alpha_ref.soft_disc(a.reshape(h, w, 4))


def _still(rng, a, amp):
    b = a.copy()
    b[..., :3] = np.clip(a[..., :3].astype(np.int64) + rng.integers(-amp, amp + 1, a[..., :3].shape), 0, 255).astype(np.uint8)
    return b


def _alpha(rng, n):
    """alpha bytes with every cutoff class well filled: a seventh transparent, half opaque, the rest anything"""
    a = rng.integers(0, 256, n)
    r = rng.random(n)
    return np.where(r < 0.15, 0, np.where(r < 0.6, 255, a)).astype(np.uint8)


def _make_images(seed, seq):
    rng = np.random.default_rng([seed, seq, 78])
    odd = rng.integers(0, 256, (61, 97, 4), dtype=np.uint8)
    odd[..., 3] = _alpha(rng, 61 * 97).reshape(61, 97)
    sprite = alpha_ref.sprite(seed=int(rng.integers(1, 1000)))
    pal = rng.integers(0, 256, (int(rng.integers(5, 10)), 4), dtype=np.uint8)
    few = pal[rng.integers(0, pal.shape[0], 50 * 80)].reshape(50, 80, 4).copy()
    few[..., 3] = 255                                             # (every pixel kept under every cutoff, as the flat one)
    flat = np.tile(rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), (48, 64, 1))
    flat[..., 3] = 255
    row = rng.integers(0, 256, (1, 131, 4), dtype=np.uint8)
    row[..., 3] = rng.choice(np.array([0, 64, 200, 255], np.uint8), (1, 131))
    col = rng.integers(0, 256, (131, 1, 4), dtype=np.uint8)
    col[..., 3] = rng.choice(np.array([0, 64, 200, 255], np.uint8), (131, 1))
    row_b, col_b = _still(rng, row, 1), _still(rng, col, 1)
    row_b[0, 5:9, 3], col_b[7:11, 0, 3] = 0, 0                    # a few pixels turn transparent
    out = [odd, _still(rng, odd, 1), sprite, _still(rng, sprite, 1), np.roll(sprite, (5, 9), (0, 1)), few, flat,
           np.zeros((30, 40, 4), np.uint8), _blobs(rng, 300, 200), _blobs(rng, 1024, 1024), row, row_b, col, col_b]
    # an importance map (surface 3), from a stream of its own: 53 x 67 noise, every alpha byte in 1 .. 255 -- every pixel is kept at
    # t <= 1, so the working image keeps its 2-D shape; the images above give the compacted, the uniform and the shrunk weights
    rng3 = np.random.default_rng([seed, seq, 79])
    wmap = rng3.integers(0, 256, (67, 53, 4), dtype=np.uint8)
    wmap[..., 3] = rng3.integers(1, 256, (67, 53))
    out.append(wmap)
    return [(k, np.ascontiguousarray(a)) for k, a in zip(IMAGE_KINDS, out)]


# ---- the stateless reference: every answer is a function of its arguments, cached per sequence -----------------------
_label_tables = collections.OrderedDict()


def _label_table(cent):
    key = cent.tobytes()
    if key not in _label_tables:
        if len(_label_tables) > 1:
            _label_tables.popitem(last=False)
        _label_tables[key] = np.full(1 << 24, -1, np.int16)
    return _label_tables[key]


def diffuse_index(rgba, cent, t):
    """(h, w) labels of KMG_MODE_DIFFUSE (include/kmeans_hip.h: lbl = the replace label of the adjusted colour c, o = its bytes),
    alpha_ref.diffuse with the label kept: an excluded pixel takes no error and passes none on, its label is that of its own colour"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    P = O.lab_to_rgba8(np.ascontiguousarray(cent[:, :3]))[:, :3].astype(np.int32)
    table = _label_table(cent)

    def labels(codes):
        got = table[codes]
        if (got < 0).any():
            new = np.unique(codes[got < 0])
            px = np.stack([new & 255, (new >> 8) & 255, (new >> 16) & 255, np.full_like(new, 255)], axis=1).astype(np.uint8)
            table[new] = O.assign(O.rgb_to_lab(px), cent).astype(np.int16)
            got = table[codes]
        return got.astype(np.int64)

    src = rgba[..., :3].astype(np.int32)
    kept = rgba[..., 3] >= t
    err = np.zeros((h + 1, w + 2, 3), np.int32)
    out = np.empty((h, w), np.int64)
    for d in range(w + 2 * (h - 1)):
        y = np.arange(max(0, (d - w + 2) // 2), min(h - 1, d // 2) + 1)
        x = d - 2 * y
        ok = (x >= 0) & (x < w)
        y, x = y[ok], x[ok]
        if y.size == 0:
            continue
        kp = kept[y, x][:, None]
        S = np.where(kp, 7 * err[y + 1, x] + 3 * err[y, x + 2] + 5 * err[y, x + 1] + err[y, x], 0)
        tq = np.clip(16 * src[y, x] + ((S + 8) >> 4), 0, 4080)
        c = ((tq + 8) >> 4).astype(np.int64)
        lbl = labels(c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16))
        out[y, x] = lbl
        err[y + 1, x + 1] = np.where(kp, tq - 16 * P[lbl], 0)
    return out


class Ref:
    """the expected results, from the reference modules; `cache` is shared by the model and the stand-ins of one sequence"""

    def __init__(self, images, cache=None):
        self.images = images
        self.cache = {} if cache is None else cache

    def _memo(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def img(self, i):
        return self.images[i][1]

    def kept(self, i, t):
        """K_i: (pixels (n, 4), sw, sh, every pixel kept) of image i after the shrink, under cutoff t"""
        def make():
            S = alpha_ref.shrink(O, self.img(i), SHRINK)
            px = S.reshape(-1, 4)
            K = px[px[:, 3] >= t] if t else px
            return np.ascontiguousarray(K), S.shape[1], S.shape[0], K.shape[0] == px.shape[0]
        return self._memo(("kept", i, t), make)

    def working(self, frames):
        """W of the frames ((image, cutoff at its add), ...): (pixels, width, height), None when empty"""
        def make():
            parts = [self.kept(i, t) for i, t in frames]
            W = np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=0)) if parts else np.zeros((0, 4), np.uint8)
            if W.shape[0] == 0:
                return None
            if len(parts) == 1 and parts[0][3]:
                return W, parts[0][1], parts[0][2]
            return W, W.shape[0], 1
        return self._memo(("W", tuple(frames)), make)

    def centroids_px(self, W, w, h, k, fid, wt=0):
        """the palette step on the working image W (w x h) with the fixed list `fid`: (k, 4) float32 in the Lloyd loop's order;
        wt: the loop is weighted by W's alpha bytes (weight_ref), the initialisation is not"""
        def make():
            if wt:
                return weight_ref.centroids_of_working(O, W, w, h, k, () if FIXED[fid] is None else np.array(FIXED[fid], np.uint8),
                                                       max_iterations=MAX_ITERATIONS, check_period=CHECK_PERIOD)[0]
            if FIXED[fid] is None:
                lab = O.rgb_to_lab(W)
                return O.lloyd(lab, O.init_centroids(lab, w, h, k), MAX_ITERATIONS, CHECK_PERIOD)[0]
            return fixed_ref.palette_centroids(O, W, w, h, k, np.array(FIXED[fid], np.uint8), max_iterations=MAX_ITERATIONS,
                                               check_period=CHECK_PERIOD)[0]
        return self._memo(("cent", hash(W.tobytes()), W.shape[0], w, h, k, fid) + (("weighted",) if wt else ()), make)

    def centroids(self, frames, k, fid, wt=0):
        W, w, h = self.working(frames)
        return self.centroids_px(W, w, h, k, fid, wt)

    # -- Lloyd objects: passes over a whole image, every pixel counted
    def lab(self, i):
        return self._memo(("lab", i), lambda: O.rgb_to_lab(self.img(i).reshape(-1, 4)))

    def q(self, i):
        return self._memo(("q", i), lambda: weight_ref.pixel_q(O, self.lab(i)))

    def alpha(self, i):
        return self.img(i).reshape(-1, 4)[:, 3]

    def assign(self, i, cent, wt=0):
        """(labels, sums) of one pass over image i; wt: the sums weigh every pixel by its alpha byte, the labels are the same"""
        def make():
            labels = O.assign(self.lab(i), cent)
            if wt:
                return labels, weight_ref.accumulate(self.q(i), self.alpha(i), labels, cent.shape[0])
            return labels, O.accumulate(self.lab(i), labels, cent.shape[0])
        return self._memo(("assign", i, cent.tobytes()) + (("weighted",) if wt else ()), make)

    def run(self, i, cent, f, wt=0):
        if wt:
            return self._memo(("run", i, cent.tobytes(), f, "weighted"),
                              lambda: weight_ref.lloyd(O, self.lab(i), self.alpha(i), cent, f, MAX_ITERATIONS, CHECK_PERIOD))
        return self._memo(("run", i, cent.tobytes(), f), lambda: fixed_ref.lloyd(O, self.lab(i), cent, f, MAX_ITERATIONS, CHECK_PERIOD))

    def seeded(self, i, k, f):
        h, w = self.img(i).shape[:2]
        seeds = fixed_ref.pins_lab(O, np.array(FIXED[3], np.uint8)[:f])
        return self._memo(("seeded", i, k, f), lambda: fixed_ref.init_centroids(O, self.lab(i), w, h, k, seeds))

    def rgba(self, rgba, cent, mode, t):
        """the RGBA8 output of an output pass over a centroid table under cutoff t"""
        def make():
            if t:
                return alpha_ref.apply(O, rgba, cent, mode, t)
            return diffuse_ref.diffuse(rgba, diffuse_ref.oracle_apply_replace(O, cent)) if mode == 3 else O.apply(rgba, cent, mode)
        return self._memo(("rgba", rgba.tobytes(), cent.tobytes(), mode, t), make)

    def index(self, rgba, cent, mode, t):
        """the index map of the same pass: (h, w) int64, k on the pixels below the cutoff"""
        def make():
            h, w = rgba.shape[:2]
            if mode == 3:
                idx = diffuse_index(rgba, cent, t)
            else:
                lab = O.rgb_to_lab(rgba.reshape(-1, 4))
                idx = (O.assign(lab, cent) if mode == 0 else O.dither(lab, w, h, cent)).astype(np.int64).reshape(h, w)
            if t:
                idx = np.where(rgba[..., 3] >= t, idx, cent.shape[0])
            return idx
        return self._memo(("index", rgba.tobytes(), cent.tobytes(), mode, t), make)

    def palette_bytes(self, cent):
        return O.lab_to_rgba8(np.ascontiguousarray(cent[:, :3]))

    def quality(self, i, t, fid, target, k_min, k_max, wt=0):
        """(k*, reached, record of W at k*) of kmg_reduce_quality's search; t: the cutoff of the working image; wt: the palettes
        are weighted, the record is the unweighted one as ever"""
        def make():
            W, _, _ = self.working(((i, t),))
            lab = O.rgb_to_lab(W)

            def record(k):
                cent = self.centroids(((i, t),), k, fid, wt)
                return error_ref.stats(O, W, O.assign(lab, cent), palette=self.palette_bytes(cent))
            k, reached, _ = error_ref.bisect(lambda kk: record(kk)[12] <= target * W.shape[0], k_min, k_max)
            return k, reached, record(k)
        return self._memo(("quality", i, t, fid, target, k_min, k_max) + (("weighted",) if wt else ()), make)

    def stats(self, src, out, palette, cutoff, what):
        pal = None if palette is None else np.ascontiguousarray(palette, np.uint8)
        return self._memo(("stats", src.tobytes(), np.ascontiguousarray(out).tobytes(), None if pal is None else pal.tobytes(), cutoff, what),
                          lambda: error_ref.stats(O, src, out, palette=pal, cutoff=cutoff, what=what))

    def palette_step(self, i, t, k):
        """(centroids, iteration count) of the default palette step on the working image of image i under cutoff t: no fixed
        colour, no weighting -- what a batched call runs for each of its images"""
        def make():
            W, w, h = self.working(((i, t),))
            lab = O.rgb_to_lab(W)
            cent, _, it = O.lloyd(lab, O.init_centroids(lab, w, h, k), MAX_ITERATIONS, CHECK_PERIOD)
            return cent, it
        return self._memo(("step", i, t, k), make)

    def lloyd_triple(self, i, k):
        """(centroids as (L, a, b, 1), iteration count) of init_centroids + run + get_centroids on the whole image i"""
        def make():
            h, w = self.img(i).shape[:2]
            cent, _, it = O.lloyd(self.lab(i), O.init_centroids(self.lab(i), w, h, k), MAX_ITERATIONS, CHECK_PERIOD)
            cent[:, 3] = 1.0
            return cent, it
        return self._memo(("triple", i, k), make)

    def find_centroids(self, pal):
        return fixed_ref.pins_lab(O, pal)

    def warm(self, i, t, prev, wt=0):
        """C_t of a warm frame: the Lloyd loop on the working image of image i under cutoff t, from all k of `prev`"""
        if wt:
            def make():
                warm4 = np.ones((prev.shape[0], 4), np.float32)
                warm4[:, :3] = np.asarray(prev, np.float32)[:, :3]
                return weight_ref.centroids_of_working(O, self.kept(i, t)[0], 0, 0, prev.shape[0], warm4=warm4, max_iterations=MAX_ITERATIONS,
                                                       check_period=CHECK_PERIOD)[0]
            return self._memo(("warm", i, t, prev.tobytes(), "weighted"), make)
        return self._memo(("warm", i, t, prev.tobytes()),
                          lambda: local_ref.warm_centroids(O, self.kept(i, t)[0], prev, MAX_ITERATIONS, CHECK_PERIOD)[0])

    def delta(self, index, canvas, k):
        return sequence_ref.delta(index, canvas, k)

    def hold(self, src, index, canvas, held, k, tol):
        return hold_ref.hold(O, src, index, canvas, held, k, tol)


def find_palette(seed, k):
    return gamut_centroids(seed, k)[1]


def target_of(max_delta_e):
    return min(int(np.floor(4096.0 * float(max_delta_e) * float(max_delta_e))), 0xFFFFFFFF)


def index_dtype(fmt):
    return np.uint8 if fmt == 1 else np.uint16


def host_format(k, t):
    """the format ImageProcessor._index_format picks"""
    return 1 if k + (1 if t else 0) <= 256 else 2


def bands_of(h, nb, order_seed):
    """nb row bands that tile h rows exactly once, in a random order: [(row0, rows), ...]"""
    nb = max(1, min(nb, h))
    rng = np.random.default_rng([order_seed, h, nb])
    cuts = sorted(rng.choice(np.arange(1, h), nb - 1, replace=False).tolist()) if nb > 1 else []
    edges = [0] + cuts + [h]
    bands = [(edges[j], edges[j + 1] - edges[j]) for j in range(nb)]
    return [bands[int(j)] for j in rng.permutation(nb)]


# ---- the model: legality state (dry) and, numeric, the expected results -----------------------------------------------
class LSlot:
    def __init__(self, k):
        self.k, self.f = k, 0
        self.cent = None
        self.nconv = None
        self.acc = None
        self.bind = None          # image index the object may be bound to
        self.w = 0                # kmg_lloyd_set_weighting
        # who holds the binding, where the model knows: None (nobody, or the library at most), "init" (the initialisation, under the
        # forced colour table), "caller" (kmg_lloyd_bind_image), "unsure" (the caller's, unless a later call of the library re-bound)
        self.owner = None


class SSlot:
    def __init__(self):
        self.frames = []          # (image, cutoff at the add): max(t, 1) when weighting was on at the add
        self.wadd = []            # the weighting at each add (coverage only: the cutoff above is all an add keeps of it)
        self.out = None           # dict(t, k, cent, mode, fmt, fam, canvas, held, last)


class Model:
    def __init__(self, images, numeric, cache=None):
        self.images, self.numeric = images, numeric
        self.ref = Ref(images, cache)
        self.t, self.fid, self.strategy = 0, 0, 0
        self.w = 0                    # kmg_processor_set_weighting
        self.lloyd = [None, None]
        self.seq = [None, None]
        self.pairs = [None, None]     # dict(fam, fmt, k, seed, mode, canvas, held, last)
        self.rec = error_ref.ZERO
        self.cpairs = [None, None]    # dict(fam, fmt, k, offs, pseed, shown, held)
        self.urec = [None, None]      # dict(k, counts, palette): the caller's usage records
        self.tables = [None, None]    # dict(k, remap, palette, info): the plans kept
        self.bad = 0                  # the running bad-pixel count of kmg_dev_index_remap

    def n_kept(self, i, t):
        """kept pixels of image i (before the shrink: the large images keep an opaque disc whatever the shrink does to its edge)"""
        a = self.images[i][1]
        return int((a[..., 3] >= t).sum()) if t else a.shape[0] * a.shape[1]

    def wc(self):
        """the cutoff of a working image made now: a pixel of weight 0 is never kept"""
        return max(self.t, 1) if self.w else self.t

    def seq_pixels(self, S):
        return sum(min(self.n_kept(i, t), 65536) for i, t in self.seq[S].frames)

    def frames_of(self, S):
        return tuple(self.seq[S].frames)


def lloyd_step(s, sums):
    """one update of a Lloyd object with n_fixed = s.f from `sums`"""
    s.cent, s.nconv = fixed_ref.step(O, sums, s.cent, s.f)


# ---- the generator --------------------------------------------------------------------------------------------------
def generate(seed, seq, n_ops=None, surface=1):
    """one sequence: a list of plain tuples.  surface 1: the calls up to the lossy delta frames, 150 ops; surface 2: those plus
    per-frame palettes, colour-keyed canvases and the index-map optimisation (SURFACE_2_OPS ops); surface 3: those plus alpha
    weighting on the processor and on the Lloyd objects (SURFACE_3_OPS random ops, then the motifs); surface 4: those plus the
    batched calls (fewer of the older motifs, the seven of the batches, and random draws -- nearly half of them batches -- until
    the list has SURFACE_4_OPS ops: the motifs' ops count, as on every surface, so most of a sequence is directed).  The
    lists of surfaces 1 to 3 never change: tests/test_session_model.py pins their hashes"""
    n_ops = {1: 150, 2: SURFACE_2_OPS, 3: SURFACE_3_OPS, 4: SURFACE_4_OPS}[surface] if n_ops is None else n_ops
    refusals = {1: REFUSALS_1, 2: REFUSALS, 3: REFUSALS + REFUSALS_3, 4: REFUSALS + REFUSALS_3 + REFUSALS_4}[surface]
    rng = np.random.default_rng([seed, seq, 3] if surface == 1 else [seed, seq, 3, surface])
    images = make_images(seed, seq)
    m = Model(images, numeric=False)
    ops = []

    def emit(op):
        ops.append(op)
        apply_op(m, op)

    def rint(a, b):
        return int(rng.integers(a, b))

    def pick(xs, p=None):
        return xs[int(rng.choice(len(xs), p=p))]

    def st():
        return rint(0, 2)

    def pick_k(classes=(0, 1, 2, 3, 4), p=(0.15, 0.4, 0.25, 0.1, 0.1), lo=1, hi=512):
        for _ in range(50):
            c = pick(list(classes), [x / sum(p[:len(classes)]) for x in p[:len(classes)]])
            a, b = K_CLASSES[c]
            k = pick([a, b]) if rng.random() < 0.3 else rint(a, b + 1)
            if lo <= k <= hi:
                return k
        return max(lo, min(hi, 8))

    def cap_k(n):
        """the largest k the reference answers in reasonable time for a palette step on n pixels under the current fixed list (its
        seeded initialisation is a Python loop over pixels x centroids)"""
        if m.fid:
            return max(200000 // max(n, 1), 1)
        return 512 if n <= 8000 else 256 if n <= 70000 else 32

    def host_image():
        """an image for a host call: kept pixels under the current cutoff, the 2^20 one only under the forced colour table"""
        pool = [ODD, SPRITE, 4, FEW, FLAT, BIG, ROW, COL] + ([MEGA] if m.strategy == 2 else []) + ([MAP, MAP] if surface >= 3 else [])
        for _ in range(20):
            i = pick(pool)
            if m.n_kept(i, m.wc()) > 0:
                return i
        return FLAT

    def host_k(i, fmt8=False):
        f = n_fixed_of(m.fid)
        hi = min(cap_k(min(m.n_kept(i, m.t), 65536)), 255 + (0 if m.t else 1) if fmt8 else 512)
        if i == MEGA:
            hi = min(hi, 32)
        return None if hi < max(f, 1) else pick_k(lo=max(f, 1), hi=hi)

    def switches():
        if surface >= 3 and rng.random() < 0.35:          # the weighting, and a palette step that sees it
            emit(("weight", 1 - m.w))
            if rng.random() < 0.6:
                emit(("palette", pick([SPRITE, MAP, ODD]), n_fixed_of(m.fid) + rint(1, 7)))
            return
        c = rng.random()
        if c < 0.45:
            emit(("cutoff", pick([x for x in CUTOFFS if x != m.t])))
        elif c < 0.8:
            emit(("fixed", 0 if m.fid and rng.random() < 0.5 else pick([x for x in range(4) if x != m.fid])))
            if rng.random() < 0.7:                        # the next palette step sees the new list, or none
                emit(("palette", pick([FEW, FLAT]), n_fixed_of(m.fid) + rint(1, 7)))
        else:
            emit(("strategy", pick([x for x in STRATEGIES if x != m.strategy], None)))

    def host():
        c = rng.random()
        i = host_image()
        if c < 0.12:
            k = host_k(i)
            if k:
                emit(("palette", i, k))
        elif c < 0.27:
            k = host_k(i)
            mode = rint(0, 4)
            if k and (i != MEGA or mode < 2):
                emit(("reduce", i, k, mode if i not in (BIG,) or mode != 3 else 0))
        elif c < 0.5:
            k = host_k(i)
            mode = pick([0, 1, 3]) if i not in (MEGA, BIG) else pick([0, 1])
            if k:
                emit(("reduce_indexed", i, k, mode, int(rng.random() < 0.5)))
        elif c < 0.6:
            if i in (MEGA, BIG):
                i = ODD
            emit(("find", i, pick_k(hi=300), rint(0, 4), rint(0, 1 << 30)))
        elif c < 0.75:
            if i in (MEGA, BIG):
                i = SPRITE
            emit(("find_indexed", i, pick_k(), pick([0, 1, 3]), rint(0, 1 << 30)))
        else:
            f = n_fixed_of(m.fid)
            if i == MEGA:
                i = BIG if m.n_kept(BIG, m.t) else FLAT
            if cap_k(min(m.n_kept(i, m.t), 65536)) >= max(12, f):
                k_min = max(pick([1, 2, 3]), f)
                emit(("quality", i, pick([1.5, 4.0, 9.0, 30.0]), k_min, pick([max(k_min, 6), 12]), pick([0, 1, 3]) if i != BIG else 0,
                      int(rng.random() < 0.6), int(rng.random() < 0.5)))

    def device():
        c = rng.random()
        i = pick([ODD, 1, SPRITE, 3, 4, FEW, FLAT, ROW, COL])
        if c < 0.3:
            mode = rint(0, 4)
            fmt = pick([None, 1, 2]) if mode != 2 else None
            k = pick_k(hi=255 + (0 if m.t else 1)) if fmt == 1 else pick_k(hi=400)
            emit(("apply", i, mode, fmt, k, rint(0, 1 << 30), st()))
        elif c < 0.5:
            mode = pick([0, 1, 3])
            fmt = pick([None, 1, 2])
            t_after = pick([x for x in CUTOFFS if x != m.t])
            # (the plan keeps the cutoff it was made under: INDEX8 is sized for the cutoff of its creation)
            k = pick_k(hi=255 + (0 if m.t else 1)) if fmt == 1 else pick_k(hi=400)
            emit(("apply_plan", i, mode, fmt, k, rint(0, 1 << 30), t_after, st()))
        elif c < 0.58:
            emit(("compact", i, pick(list(CUTOFFS)), st()))
        elif c < 0.8:
            if m.strategy == 2 and rng.random() < 0.3:
                i = MEGA
            fmt = pick([None, 1, 2])
            cut = pick([m.t, 0, 128])
            k = pick_k(hi=255) if fmt == 1 else pick_k(hi=32 if i == MEGA else 400)
            emit(("compare_device", i, pick([0, 1]), fmt, k, rint(0, 1 << 30), rint(1, 4), rint(0, 1 << 30), cut, pick([1, 2, 3, 3]),
                  int(rng.random() < 0.6), st()))
        else:
            P = rint(0, 2)
            if m.pairs[P] is None or rng.random() < 0.2:
                fmt = pick([1, 2])
                emit(("pair_open", P, rint(0, len(FAMILIES)), fmt, pick_k(hi=255) if fmt == 1 else pick_k(hi=400), rint(0, 1 << 30),
                      pick([0, 1, 3])))
            pr = m.pairs[P]
            for _ in range(rint(2, 5)):
                emit(("pair_frame", P, pick(list(FAMILIES[pr["fam"]])), pick([None] + list(TOLERANCES)), rint(1, 4), rint(0, 1 << 30), st()))

    def lloyd_ops():
        L = rint(0, 2)
        s = m.lloyd[L]
        if s is None:
            emit(("l_new", L, pick_k()))
            return
        if surface >= 3 and rng.random() < 0.22:
            return l_weight_ops(L)
        c = rng.random()
        if c < 0.04:
            emit(("l_close", L))
            return
        if c < 0.12 or (s.f and c < 0.3):
            emit(("l_re", L, pick_k()))
            if s.f:                                       # nothing is frozen in the new object, whatever its block's last owner froze
                emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
                emit(("l_assign_update", L, pick([ODD, FEW, ROW]), 1, 1, st()))
            return
        i = pick([ODD, SPRITE, FEW, FLAT, BIG, ROW] + ([MAP] if surface >= 3 else []))
        n = images[i][1].shape[0] * images[i][1].shape[1]
        if s.cent is None or c < 0.24:
            if n * s.k <= 300000 and rng.random() < 0.7:
                f = min(pick([0, 1, 3, 8]), s.k)
                emit(("l_init", L, i, f, st()))
                if f:
                    emit(("l_fix", L, pick([f, f, min(f, 1)])))
            else:
                emit(("l_set", L, pick(["rand", "dup", "init"]), rint(0, 1 << 30), pick([ODD, FEW])))
            return
        if c < 0.34:
            emit(("l_fix", L, 0 if s.f and rng.random() < 0.6 else pick([min(s.k, 1), min(s.k, 2), min(s.k, 3), min(s.k, 8)])))
            if rng.random() < 0.6:
                emit(("l_assign_update", L, pick([ODD, FEW, ROW]), 0, 1, st()))
            return
        if c < 0.44:
            emit(("l_update", L, st()))
        elif c < 0.58:
            emit(("l_assign_update", L, i, rint(0, 2), rint(0, 2), st()))
        elif c < 0.7:
            if rng.random() < 0.5:
                if not s.w:
                    emit(("l_bind", L, i, st()))
                elif s.k <= 256:
                    emit(("refuse", "weighted_bind", L, i))
            emit(("l_iterate", L, i, rint(1, 4), st()))
        elif c < 0.82:
            emit(("l_run", L, i, rint(0, 2), st()))
        elif c < 0.92 and s.k <= 256:
            if s.w:                                       # a weighted object has no colour-table route
                emit(("refuse", pick(["weighted_lftu", "weighted_accumulate_into"]), L, i))
                emit(("l_assign", L, i, st()))
            else:
                emit(("l_lftu", L, i, st()))
        else:
            emit(("l_assign", L, i, st()))
        if m.lloyd[L].nconv is not None and rng.random() < 0.3:
            emit(("l_conv", L, st()))

    def seq_k(S, fmt):
        f = n_fixed_of(m.fid)
        hi = min(cap_k(m.seq_pixels(S)), 255 if fmt == 1 else 512)
        return None if hi < max(f, 1) else pick_k(lo=max(f, 1), hi=hi)

    def sequence_ops():
        S = rint(0, 2)
        q = m.seq[S]
        if q is None:
            emit(("s_new", S))
            return
        c = rng.random()
        if c < 0.04:
            emit(("s_close", S))
            return
        if c < 0.3 or not q.frames:
            if len(q.frames) >= 5:
                emit(("s_clear", S))
            i = pick([ODD, 1, SPRITE, 3, 4, FEW, FLAT, BIG, ROW, COL, CLEAR], None)
            if i == CLEAR and m.t == 0:
                i = SPRITE
            emit(("s_add", S, i, int(i != BIG and rng.random() < 0.4), st()))
            if rng.random() < 0.4:
                emit(("s_info", S))
            return
        if c < 0.36:
            emit(("s_clear", S))
            if rng.random() < 0.4:                        # a first frame that loses pixels, a clear, then one whole frame
                if m.t == 0:
                    emit(("cutoff", pick([1, 128, 255])))
                emit(("s_add", S, SPRITE, 0, 0))
                emit(("s_clear", S))
                if m.fid:
                    emit(("fixed", 0))
                emit(("s_add", S, FEW, rint(0, 2), st()))
                emit(("s_centroids", S, rint(3, 7)))
                return
            emit(("s_info", S))
            if rng.random() < 0.7:                        # one whole frame after the clear: an image of its own size again
                if m.fid and rng.random() < 0.5:
                    emit(("fixed", 0))                    # (with a fixed colour the size does not enter the initialisation)
                emit(("s_add", S, pick([FEW, SPRITE, ODD]) if m.t == 0 else FEW, 0, 0))
                k = seq_k(S, 2)
                if k:
                    emit(("s_centroids", S, min(k, 24)))
            return
        if m.seq_pixels(S) == 0:
            emit(("refuse", "empty_sequence", S, 4))
            emit(("s_add", S, SPRITE if m.n_kept(SPRITE, m.t) else FLAT, 0, 0))
            return
        if c < 0.46:
            k = seq_k(S, 2)
            if k:
                emit(("s_centroids" if rng.random() < 0.5 else "s_palette", S, k))
            return
        if q.out is None or q.out.get("local") or c < (0.6 if q.out["last"] else 0.5):
            mode = rint(0, 4)
            fmt = pick([1, 1, 2]) if mode != 2 else 0
            if mode != 2 and rng.random() < 0.12:
                fmt = 0
            k = seq_k(S, fmt)
            if k:
                fam = q.out["fam"] if q.out is not None and rng.random() < 0.6 else rint(0, len(FAMILIES))
                emit(("s_output", S, k, mode, fmt, fam))
                if fmt:                                   # against the fresh canvas the first delta is the full map
                    emit(("s_frame", S, pick(list(FAMILIES[fam])), 1, pick([None, 40])))
            return
        if c < 0.64:
            emit(("s_end", S))
            return
        fam = FAMILIES[q.out["fam"]]
        if q.out["fmt"] and rng.random() < 0.5:           # another frame, the base frame, then its still copy within a tolerance
            emit(("s_frame", S, fam[-1], 1, None))
            emit(("s_frame", S, fam[0], rint(0, 2), None))
            emit(("s_frame", S, fam[1], 1, pick([40, 4096])))
            if rng.random() < 0.5:
                emit(("s_frame", S, fam[0], 1, None))
            return
        if q.out["fmt"] and rng.random() < 0.4:           # rewritten under a tolerance: the anchor moves with the pixel
            emit(("s_frame", S, fam[0], 1, None))
            emit(("s_frame", S, fam[-1], 1, 40))
            emit(("s_frame", S, fam[1], 1, 4096))
            return
        for _ in range(rint(1, 4)):
            if m.seq[S].out["fmt"] == 0:
                emit(("s_frame", S, pick(list(fam)), 0, None))
            else:
                tol = pick([None, None, None] + list(TOLERANCES))
                emit(("s_frame", S, pick(list(fam)), 1 if tol is not None or rng.random() < 0.8 else 0, tol))

    def refusal(what=None):
        what = pick(list(refusals)) if what is None else what
        if what in REFUSALS_2:
            return refusal_2(what)
        if what in REFUSALS_3:
            return refusal_3(what)
        if what in REFUSALS_4:
            return refusal_4(what)
        f = n_fixed_of(m.fid)
        if what.startswith("k_below_fixed") or what == "octree_fixed":
            if f < 2:
                emit(("fixed", pick([2, 3])))
                f = n_fixed_of(m.fid)
            i = SPRITE if m.n_kept(SPRITE, m.t) else FLAT
            if what == "k_below_fixed_sequence":
                S = rint(0, 2)
                if m.seq[S] is None:
                    emit(("s_new", S))
                if m.seq_pixels(S) == 0:
                    emit(("s_add", S, i, 0, 0))
                if m.seq_pixels(S) > 20000:
                    return
                emit(("refuse", what, S, f - 1))
                emit(("s_palette", S, f + 1))
            else:
                emit(("refuse", what, i, f - 1 if what != "octree_fixed" else f + 2))
                emit(("palette" if what != "k_below_fixed_reduce" else "reduce", i, f + 2) + ((0,) if what == "k_below_fixed_reduce" else ()))
            return
        if what == "index8_full":
            i = pick([ODD, FLAT])
            emit(("refuse", what, i, 256 if m.t else 257))
            emit(("apply", i, 0, 1, 255 if m.t else 256, rint(0, 1 << 30), st()))
            return
        if what == "meld_indexed":
            emit(("refuse", what, FLAT, 5))
            emit(("apply", FLAT, 0, 2, 5, rint(0, 1 << 30), st()))
            return
        if what == "empty_sequence":
            if m.t == 0:
                emit(("cutoff", pick([1, 128, 255])))
            S = rint(0, 2)
            emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
            emit(("s_add", S, CLEAR, 0, 0))
            emit(("refuse", what, S, 4))
            emit(("s_add", S, FLAT, 0, 0))
            emit(("s_palette", S, 2 + n_fixed_of(m.fid)))
            return
        # the frame refusals
        S = rint(0, 2)
        if m.seq[S] is None:
            emit(("s_new", S))
        if m.seq_pixels(S) == 0:
            emit(("s_add", S, SPRITE if m.n_kept(SPRITE, m.t) else FLAT, 0, 0))
        if cap_k(m.seq_pixels(S)) < max(f, 1) + 1:
            return
        k = max(f, 1) + 1
        if what == "frame_no_output":
            if m.seq[S].out is not None:
                emit(("s_end", S))
            emit(("refuse", what, S, SPRITE))
            emit(("s_output", S, k, 0, 1, 1))
            emit(("s_frame", S, SPRITE, 1, None))
        else:
            emit(("s_output", S, k, 0, 0 if what != "lossy_without_delta" else 1, 1))
            emit(("refuse", what, S, 3))
            emit(("s_frame", S, 3, 0, None))

    # ---- motifs: short directed passages, most of them in every sequence, at random places between the random ops
    def small_sequence(S):
        """sequence S with a small working sequence of kept pixels, whatever it held"""
        emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
        emit(("s_add", S, SPRITE if m.n_kept(SPRITE, m.t) else FEW, rint(0, 2), st()))

    def motif_reoutput():
        """an output with frames, ended, a Lloyd object in the returned block, an output of another k and format: a fresh canvas"""
        S, f = rint(0, 2), n_fixed_of(m.fid)
        small_sequence(S)
        emit(("s_output", S, f + rint(2, 30), pick([0, 1, 3]), 1, 1))
        for i, tol in ((2, None), (3, 40), (4, 4096), (2, None))[:rint(2, 5)]:
            emit(("s_frame", S, i, 1, tol))
        if rng.random() < 0.6:
            emit(("s_end", S))
            if m.lloyd[0] is None and rng.random() < 0.7:
                emit(("l_new", 0, pick_k()))
                emit(("l_set", 0, "rand", rint(0, 1 << 30), ODD))
                emit(("l_run", 0, FEW, 1, st()))
                emit(("l_close", 0))
        emit(("s_output", S, f + rint(2, 30) if rng.random() < 0.5 else min(f + rint(257, 400), cap_k(m.seq_pixels(S))), pick([0, 1]), 2, 1))
        emit(("s_frame", S, pick([2, 3]), 1, pick([None, 40])))

    def motif_anchor():
        """exact and lossy frames alternate: the held source is the frame that wrote the pixel, and moves when the pixel is rewritten"""
        S, f = rint(0, 2), n_fixed_of(m.fid)
        small_sequence(S)
        emit(("s_output", S, f + rint(2, 40), pick([0, 1, 3]), pick([1, 2]), 1))
        emit(("s_frame", S, 4, 1, None))
        emit(("s_frame", S, 2, rint(0, 2), None))
        emit(("s_frame", S, 3, 1, pick([40, 4096])))
        emit(("s_frame", S, 4, 1, 40))
        emit(("s_frame", S, 3, 1, 4096))
        emit(("s_frame", S, 2, 1, None))

    def motif_growth():
        """a working sequence that outgrows its block several times, frames from both sides"""
        S = rint(0, 2)
        emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
        for i in (ROW, COL, FEW, BIG if m.fid < 2 else ODD)[:rint(3, 5)]:
            emit(("s_add", S, i, int(i != BIG and rng.random() < 0.5), st()))
        emit(("s_info", S))
        emit(("s_centroids", S, n_fixed_of(m.fid) + rint(2, 6)))

    def motif_first_frame():
        """a first frame that loses pixels, a clear, then one whole frame: an image of its own size again"""
        S = rint(0, 2)
        emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
        if m.t == 0:
            emit(("cutoff", pick([1, 128, 255])))
        emit(("s_add", S, SPRITE, 0, 0))
        emit(("s_clear", S))
        if m.fid:
            emit(("fixed", 0))                            # (with a fixed colour the size does not enter the initialisation)
        emit(("s_add", S, FEW, rint(0, 2), st()))
        emit(("s_centroids", S, rint(3, 7)))

    def motif_freeze():
        """seeds frozen and run; a new object in the same block, nothing frozen; frozen, unfrozen, updated"""
        L = rint(0, 2)
        emit(("l_new" if m.lloyd[L] is None else "l_re", L, rint(4, 40)))
        emit(("l_init", L, pick([FEW, ROW, SPRITE]), 3, st()))
        emit(("l_fix", L, 3))
        for carrier in rng.permutation(5)[:rint(1, 4)]:           # every update carrier leaves the frozen three alone
            i = pick([FEW, ROW, SPRITE])
            emit([("l_run", L, i, 1, st()), ("l_update", L, st()), ("l_assign_update", L, i, 1, 1, st()), ("l_iterate", L, i, rint(1, 4), st()),
                  ("l_lftu", L, i, st())][int(carrier)])
            if m.lloyd[L].nconv is not None and rng.random() < 0.5:
                emit(("l_conv", L, st()))
        emit(("l_re", L, rint(3, 300)))
        emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
        emit(("l_assign_update", L, ODD, 1, 1, st()))
        emit(("l_fix", L, 2))
        emit(("l_fix", L, 0))
        emit(("l_assign_update", L, ODD, 0, 1, st()))

    def motif_pins():
        """pins set, a quality search, pins cleared, the same search again"""
        i = FEW
        emit(("fixed", pick([2, 3])))
        f = n_fixed_of(m.fid)
        args = (i, pick([4.0, 9.0]), f, f + 6, 0, rint(0, 2), 0)
        emit(("quality",) + args)
        emit(("fixed", 0))
        emit(("quality",) + args)
        emit(("palette", i, rint(2, 9)))

    def motif_cutoff():
        """a plan and an open output made under one cutoff, run under another: each keeps its own"""
        S, f = rint(0, 2), n_fixed_of(m.fid)
        if m.t == 0:
            emit(("cutoff", pick([1, 128, 255])))
        small_sequence(S)
        emit(("s_output", S, f + rint(2, 20), pick([0, 1, 3]), pick([1, 2]), pick([0, 1])))
        i = FAMILIES[m.seq[S].out["fam"]][0]
        emit(("apply_plan", i, pick([0, 1, 3]), pick([1, 2]), rint(2, 200), rint(0, 1 << 30), 0, st()))
        emit(("s_frame", S, i, 1, None))
        emit(("reduce_indexed", i, f + rint(2, 12), pick([0, 1, 3]), 1))

    def motif_mixed():
        """frames added under different cutoffs: each keeps the pixels its own cutoff kept"""
        S = rint(0, 2)
        emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
        for i in (SPRITE, ODD, 4):
            emit(("cutoff", pick([x for x in CUTOFFS if x != m.t])))
            if m.n_kept(i, m.t):
                emit(("s_add", S, i, rint(0, 2), st()))
        emit(("s_info", S))
        k = seq_k(S, 2)
        if k:
            emit(("s_palette" if rng.random() < 0.5 else "s_centroids", S, min(k, 40)))

    def motif_refusals():
        for j in rng.permutation(len(REFUSALS_1))[:3]:
            refusal(REFUSALS_1[int(j)])
        if surface >= 2:
            for j in rng.permutation(len(REFUSALS_2))[:4]:
                refusal(REFUSALS_2[int(j)])
        if surface >= 3:
            for j in rng.permutation(len(REFUSALS_3))[:4]:
                refusal(REFUSALS_3[int(j)])
        if surface >= 4:
            for j in rng.permutation(len(REFUSALS_4))[:4]:
                refusal(REFUSALS_4[int(j)])


    # ---- surface 2: per-frame palettes, colour-keyed canvases, index-map optimisation -------------------------------------
    def fam_pixels(fam):
        a = images[LOCAL_FAMILIES[fam][0]][1]
        return a.shape[0] * a.shape[1]

    def local_k(fam, fmt):
        f = n_fixed_of(m.fid)
        hi = min(cap_k(fam_pixels(fam)), 255 if fmt == 1 else 512)
        return None if hi < max(f, 1) else pick_k(p=(0.15, 0.42, 0.25, 0.1, 0.08), lo=max(f, 1), hi=hi)

    def need_seq(S):
        if m.seq[S] is None:
            emit(("s_new", S))

    def open_local(S, fam=None, k=None, fmt=None, warm=None, mode=None):
        need_seq(S)
        fam = rint(0, len(FAMILIES)) if fam is None else fam
        warm = int(rng.random() < 0.5) if warm is None else warm
        if warm and m.fid:
            emit(("fixed", 0))
        fmt = pick([1, 1, 2]) if fmt is None else fmt
        k = local_k(fam, fmt) if k is None else k
        if k is None or k < n_fixed_of(m.fid) or (m.fid and k > cap_k(fam_pixels(fam))):
            emit(("fixed", 0))
            k = rint(2, 24) if k is None else k
        emit(("s_output_local", S, k, pick([0, 1, 3]) if mode is None else mode, fmt, fam, warm))

    def frame_local(S, i, delta=1, tol=None):
        o = m.seq[S].out
        if m.fid and not o["warm"] and o["k"] >= n_fixed_of(m.fid) and o["k"] > cap_k(fam_pixels(o["fam"])):
            emit(("fixed", 0))                                # (the seeded initialisation of the reference is a Python loop)
        emit(("s_frame_local", S, i, delta, tol))

    def local_ops():
        S = rint(0, 2)
        q = m.seq[S]
        if q is None or q.out is None or not q.out.get("local") or rng.random() < 0.2:
            open_local(S)
        o = m.seq[S].out
        fam = LOCAL_FAMILIES[o["fam"]]
        for _ in range(rint(1, 4)):
            tol = pick([None, None] + list(TOLERANCES))
            frame_local(S, pick(list(fam)), 1 if tol is not None or rng.random() < 0.8 else 0, tol)
        if rng.random() < 0.25:
            s_index_ops(S)

    def cpair_ops(P=None, n=None):
        P = rint(0, 2) if P is None else P
        if m.cpairs[P] is None or rng.random() < 0.2:
            fmt = pick([1, 2])
            emit(("cpair_open", P, rint(0, len(FAMILIES)), fmt, pick_k(hi=255) if fmt == 1 else pick_k(p=(0.15, 0.42, 0.25, 0.1, 0.08), hi=400),
                  pick(list(CPAIR_OFFSETS))))
        pr = m.cpairs[P]
        for _ in range(rint(2, 5) if n is None else n):
            pseed = pr["pseed"] if pr["pseed"] is not None and rng.random() < 0.45 else rint(0, 1 << 30)
            emit(("cpair_frame", P, pick(list(FAMILIES[pr["fam"]])), pseed, pick([None, None] + list(TOLERANCES)), rint(1, 4), rint(0, 1 << 30), st()))

    def small_image():
        return pick([ODD, 1, SPRITE, 3, 4, FEW, FLAT, ROW, COL])

    def usage_op(i=None, rec=None, fresh=None, fmt=None, k=None, nb=None):
        i = small_image() if i is None else i
        rec = rint(0, 2) if rec is None else rec
        u = m.urec[rec]
        fresh = int(u is None or rng.random() < 0.5) if fresh is None else fresh
        fmt = pick([1, 2]) if fmt is None else fmt
        if not fresh:
            k = u["k"]
        elif k is None:
            k = pick_k(hi=256 - (1 if m.t else 0)) if fmt == 1 else pick_k(p=(0.15, 0.42, 0.25, 0.1, 0.08), hi=512)
        if fmt == 1 and k + (1 if m.t else 0) > 256:
            fmt = 2
        emit(("usage_device", i, pick([0, 1, 3]), fmt, k, rint(0, 1 << 30), rec, rint(1, 4) if nb is None else nb, rint(0, 1 << 30), st(), fresh))

    def plan_op(rec=None, slot=None, flags=None):
        rec = pick([r for r in range(2) if m.urec[r] is not None]) if rec is None else rec
        flags = pick([0, 1, 2]) | (4 if rng.random() < 0.4 else 0) | (8 if rng.random() < 0.4 else 0) | (16 if rng.random() < 0.4 else 0) \
            if flags is None else flags
        emit(("plan", rec, rint(0, 2) if slot is None else slot, flags))

    def remap_op(i=None, table=None, bits=None, bad_fresh=None):
        i = small_image() if i is None else i
        bits = pick(list(BITS)) if bits is None else bits
        slots = [t for t in range(2) if m.tables[t] is not None]
        if table is None:
            table = pick(slots) if slots and rng.random() < 0.5 else ("rand", rint(0, 1 << 30))
        fmt = pick([1, 2])
        if isinstance(table, int):
            k = m.tables[table]["k"]
        else:
            k = pick_k(hi=256 - (1 if m.t else 0)) if fmt == 1 else pick_k(p=(0.15, 0.42, 0.25, 0.1, 0.08), hi=512)
        if fmt == 1 and k + (1 if m.t else 0) > 256:
            fmt = 2
        in_place = int(bits == 8 * fmt and rng.random() < 0.6)
        emit(("remap_device", i, pick([0, 1, 3]), fmt, k, rint(0, 1 << 30), table, bits, in_place,
              int(rng.random() < 0.4) if bad_fresh is None else bad_fresh, st()))

    def optimize_op(i=None, flags=None):
        for _ in range(20):
            i = pick([ODD, SPRITE, 4, FEW, FLAT, ROW, COL]) if i is None else i
            if m.n_kept(i, m.t) > 0:
                break
            i = None
        if i is None:
            i = FLAT
        k = host_k(i)
        if not k:
            return
        flags = pick([0, 1, 2]) | (4 if rng.random() < 0.3 else 0) | (8 if rng.random() < 0.4 else 0) | (16 if rng.random() < 0.4 else 0) \
            if flags is None else flags
        emit(("optimize", i, k, pick([0, 1, 3]), flags, pick([0, 8 * host_format(k, m.t)])))

    def s_index_ops(S):
        """the host calls on a map a frame of S returned"""
        o = m.seq[S].out
        if o is None or not o["coded"]:
            return
        rec = rint(0, 2)
        u = m.urec[rec]
        emit(("s_usage", S, rec, int(u is None or u["k"] != o["k"] or rng.random() < 0.4), rint(0, len(o["coded"]))))
        if rng.random() < 0.7:
            slot = rint(0, 2)
            emit(("plan", rec, slot, pick([0, 1, 2]) | (8 if rng.random() < 0.5 else 0) | (16 if rng.random() < 0.3 else 0)))
            emit(("s_remap", S, slot, pick([8, 16] if o["k"] > 15 else [4, 8, 16]), rint(0, len(o["coded"])), 0))

    def index_ops():
        c = rng.random()
        if c < 0.3 or (m.urec[0] is None and m.urec[1] is None):
            usage_op()
        elif c < 0.45:
            plan_op()
        elif c < 0.7:
            remap_op()
        elif c < 0.85:
            optimize_op()
        else:
            S = rint(0, 2)
            if m.seq[S] is not None:
                s_index_ops(S)

    def surface_2_ops():
        c = rng.random()
        if c < 0.4:
            local_ops()
        elif c < 0.6:
            cpair_ops()
        else:
            index_ops()

    def refusal_2(what):
        S = rint(0, 2)
        if what in ("shared_frame_on_local", "local_tolerance_without_delta", "warm_with_fixed"):
            open_local(S, fam=pick([0, 1]), k=rint(2, 20), warm=int(what == "warm_with_fixed"))
            i = LOCAL_FAMILIES[m.seq[S].out["fam"]][0]
            if what == "warm_with_fixed":
                frame_local(S, i)
                emit(("fixed", pick([1, 2, 3])))
            emit(("refuse", what, S, i))
            if what == "warm_with_fixed":
                emit(("fixed", 0))
            frame_local(S, LOCAL_FAMILIES[m.seq[S].out["fam"]][1], int(what != "local_tolerance_without_delta"), None)
        elif what == "local_frame_on_shared":
            small_sequence(S)
            emit(("s_output", S, n_fixed_of(m.fid) + rint(2, 12), pick([0, 1]), 1, 1))
            emit(("refuse", what, S, SPRITE))
            emit(("s_frame", S, SPRITE, 1, None))
        elif what == "local_frame_no_output":
            need_seq(S)
            if m.seq[S].out is not None:
                emit(("s_end", S))
            emit(("refuse", what, S, ODD))
            open_local(S, fam=0, k=rint(2, 20))
            frame_local(S, ODD)
        elif what in ("local_meld", "local_index8_k256"):
            need_seq(S)
            emit(("refuse", what, S, 256 if what == "local_index8_k256" else 5))       # (the refused begin has ended what was open)
            open_local(S, fam=1, k=255 if what == "local_index8_k256" and not m.fid else rint(2, 20), fmt=1)
            frame_local(S, SPRITE)
        elif what in ("plan_indices_above_k", "plan_empty_record"):
            rec = rint(0, 2)
            if m.urec[rec] is None:
                usage_op(rec=rec, fresh=1)
            emit(("refuse", what, rec, 0))
            plan_op(rec=rec)
        elif what == "optimize_bits_too_narrow":
            i = FEW if m.n_kept(FEW, m.t) else FLAT
            k = max(n_fixed_of(m.fid), 3) + rint(0, 6)
            emit(("refuse", what, i, k))
            emit(("optimize", i, k, 0, 4, 0))
        else:
            assert what == "remap_bad_bits", what
            emit(("refuse", what, FLAT, pick([0, 3, 5, 32])))
            remap_op(i=FLAT)

    def restore_cutoff(t):
        if m.t != t:
            emit(("cutoff", t))

    def motif_warm_cutoff():
        """a warm output across a cutoff switch and back: each frame's working image is that of the cutoff read at its call"""
        S, t0 = rint(0, 2), m.t
        fam = pick([0, 1])
        open_local(S, fam=fam, k=rint(3, 24), warm=1)
        F = LOCAL_FAMILIES[fam]
        frame_local(S, F[0])
        frame_local(S, F[1], 1, pick([None, 40]))
        emit(("cutoff", pick([x for x in CUTOFFS if x != m.t])))
        frame_local(S, F[-1])
        emit(("cutoff", t0))
        frame_local(S, F[0], 1, pick([None, 4096]))

    def motif_refused_warm():
        """frame / refused frame / frame on a warm output: the refusal changes nothing, the frame after it is warm; a frame that
        fails in its palette step makes the next one cold"""
        S, t0 = rint(0, 2), m.t
        open_local(S, fam=1, k=rint(3, 16), warm=1, mode=pick([0, 1]))
        frame_local(S, SPRITE)
        emit(("fixed", pick([1, 2, 3])))
        emit(("s_frame_local", S, 3, 1, None))               # -5: fixed colours on a warm output
        emit(("fixed", 0))
        frame_local(S, 3)
        open_local(S, fam=0, k=2, warm=0, fmt=1)
        frame_local(S, ODD)
        emit(("fixed", 3))
        emit(("s_frame_local", S, 1, 1, None))               # -1: k below the fixed colours
        emit(("fixed", 0))
        frame_local(S, 1, 1, 40)
        restore_cutoff(0)
        open_local(S, fam=len(FAMILIES), k=rint(2, 5), warm=1, fmt=1)
        frame_local(S, CLEAR)
        emit(("cutoff", pick([1, 128, 255])))
        emit(("s_frame_local", S, CLEAR, 1, None))           # -1: no pixel reaches the cutoff
        emit(("cutoff", 0))
        frame_local(S, CLEAR)
        emit(("s_end", S))
        restore_cutoff(t0)

    def motif_used_block():
        """a shared output ended, a Lloyd object run and closed, a local output of a smaller k in the block that came back, a lossy
        first frame: shown is filled at the begin, the held source is not and must not be read"""
        S, f = rint(0, 2), n_fixed_of(m.fid)
        small_sequence(S)
        emit(("s_output", S, f + rint(20, 30), pick([0, 1]), pick([1, 2]), 1))
        emit(("s_frame", S, SPRITE, 1, None))
        emit(("s_frame", S, 3, 1, 40))
        emit(("s_end", S))
        if m.lloyd[0] is None:
            emit(("l_new", 0, pick_k(hi=64)))
            emit(("l_set", 0, "rand", rint(0, 1 << 30), ODD))
            emit(("l_run", 0, FEW, 1, st()))
            emit(("l_close", 0))
        open_local(S, fam=1, k=max(f, 1) + rint(1, 8), fmt=1)
        frame_local(S, SPRITE, 1, 40)
        frame_local(S, 3, 1, 4096)
        frame_local(S, 4, 1, None)
        # ... and a second begin on the same sequence: nothing shown, nothing to start warm from
        open_local(S, fam=1, k=m.seq[S].out["k"], fmt=1, warm=m.seq[S].out["warm"], mode=m.seq[S].out["mode"])
        frame_local(S, 3, 1, 40)
        frame_local(S, SPRITE)

    def motif_lossy_full():
        """a lossy frame whose sprite shifted comes back in full; an exact delta frame and a lossy frame after it"""
        S, t0 = rint(0, 2), m.t
        if m.t == 0:
            emit(("cutoff", pick([1, 128, 255])))
        open_local(S, fam=1, k=rint(3, 24))
        frame_local(S, SPRITE)
        frame_local(S, 4, 1, pick([40, 4096]))
        frame_local(S, 3, 1, None)
        frame_local(S, SPRITE, 1, 4096)
        frame_local(S, 4, 1, 400000)
        frame_local(S, 3, 1, 40)
        restore_cutoff(t0)

    def motif_local_shared_local():
        """local / shared / local on one Sequence, with the two cross refusals, which leave the output open"""
        S = rint(0, 2)
        small_sequence(S)
        open_local(S, fam=1, k=rint(3, 16))
        frame_local(S, SPRITE)
        emit(("refuse", "shared_frame_on_local", S, 3))
        frame_local(S, 3)
        emit(("s_output", S, n_fixed_of(m.fid) + rint(2, 12), pick([0, 1]), pick([1, 2]), 1))
        emit(("s_frame", S, SPRITE, 1, None))
        emit(("refuse", "local_frame_on_shared", S, 3))
        emit(("s_frame", S, 3, 1, pick([None, 40])))
        open_local(S, fam=1, k=rint(3, 16))
        frame_local(S, 4)
        frame_local(S, 3, 1, 40)

    def motif_optimize_path():
        """what `sequence --optimize` does: one usage record over the coded frames, one plan, every frame remapped"""
        S, rec, slot = rint(0, 2), rint(0, 2), rint(0, 2)
        small_sequence(S)
        emit(("s_output", S, n_fixed_of(m.fid) + rint(4, 40), pick([0, 1, 3]), 1, 1))
        for j, i in enumerate((SPRITE, 3, 4)):
            emit(("s_frame", S, i, 1, None))
            emit(("s_usage", S, rec, int(j == 0), j))
        emit(("plan", rec, slot, index_ref.ORDER_USAGE | index_ref.KEEP_TRANSPARENT))
        for j in range(3):
            emit(("s_remap", S, slot, 8, j, 1))

    def motif_records():
        """records that outlive their map: usage of A, an optimize of B, usage of C into the same record; the bad count across two
        remaps; INDEX8 at k = 256; two optimize calls in a row"""
        rec, slot = rint(0, 2), rint(0, 2)
        usage_op(i=ODD, rec=rec, fresh=1, nb=pick([2, 3]))
        optimize_op(flags=pick([1, 1 | 16]))
        usage_op(i=1, rec=rec, fresh=0, nb=pick([2, 3]))
        optimize_op(flags=pick([1, 1 | 8]))
        plan_op(rec=rec, slot=slot)
        remap_op(i=ODD, table=slot, bits=pick([8, 16]), bad_fresh=1)
        remap_op(i=ODD, table=("rand", rint(0, 1 << 30)), bits=pick([1, 2, 4]), bad_fresh=1)
        remap_op(i=ROW, table=("rand", rint(0, 1 << 30)), bits=pick([1, 2, 4]), bad_fresh=0)
        t0 = m.t
        restore_cutoff(0)
        usage_op(i=ODD, rec=1 - rec, fresh=1, fmt=1, k=256, nb=2)
        restore_cutoff(t0)

    def motif_cpair():
        """a colour-keyed canvas of the caller's on the per-pixel route and on the vector route, palettes kept and changed"""
        for P, offs in ((0, 1), (1, pick([0, 4]))):
            fmt = pick([1, 2])
            emit(("cpair_open", P, 1, fmt, rint(5, 40), offs))
            cpair_ops(P, 4)

    # ---- surface 3: alpha weighting -----------------------------------------------------------------------------------------
    def set_weight(v):
        if m.w != v:
            emit(("weight", v))

    def need_lloyd(hi=64):
        """a Lloyd slot whose object exists and has centroids"""
        L = rint(0, 2)
        if m.lloyd[L] is None:
            emit(("l_new", L, pick_k(hi=hi)))
        if m.lloyd[L].cent is None:
            emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
        return L

    def make_settable(L):
        """the setter is refused under a caller's binding: unbind first where the model knows of one or cannot rule it out"""
        if m.lloyd[L].owner in ("caller", "unsure"):
            emit(("l_unbind", L))

    def l_weight_ops(L):
        s = m.lloyd[L]
        if s.owner == "caller" and rng.random() < 0.5:
            emit(("refuse", "l_weight_under_caller_binding", L, rint(0, 2)))
        make_settable(L)
        emit(("l_weight", L, 1 - s.w if rng.random() < 0.8 else s.w))
        if s.cent is not None:
            i = pick([ODD, SPRITE, FEW, ROW, MAP, MAP])
            emit(pick([("l_assign_update", L, i, rint(0, 2), rint(0, 2), st()), ("l_run", L, i, rint(0, 2), st()), ("l_iterate", L, i, rint(1, 3), st()),
                       ("l_assign", L, i, st())]))

    def refusal_3(what):
        f = n_fixed_of(m.fid)
        if what == "weight_bad_value":                        # the old value stays in force: mostly weighting on, which a reset would show
            if rng.random() < 0.7:
                set_weight(1)
            emit(("refuse", what, pick([2, -1, 255])))
            emit(("palette", pick([SPRITE, MAP]), f + rint(2, 6)))
        elif what == "octree_weighted":                       # no fixed colours: the weighting is the only cause (octree_fixed is the other)
            if m.fid:
                emit(("fixed", 0))
            set_weight(1)
            k = rint(2, 12)
            for variant in rng.permutation(3):                # palette, reduce (nothing written), reduce_indexed
                emit(("refuse", what, SPRITE, k, int(variant)))
            emit(("palette", SPRITE, rint(2, 6)))
        elif what == "weighted_no_kept_pixel":                # no fixed colours either: k below them is refused before the image is looked at
            t0 = m.t
            if m.fid:
                emit(("fixed", 0))
            restore_cutoff(0)
            set_weight(1)
            for variant in rng.permutation(3):
                emit(("refuse", what, int(variant)))
            emit(("palette", FLAT, 2))
            restore_cutoff(t0)
        elif what == "l_weight_bad_value":
            L = need_lloyd()
            emit(("refuse", what, L, pick([2, -1])))
            emit(("l_assign", L, pick([ODD, MAP]), st()))
        elif what == "l_weight_under_caller_binding":
            L = need_lloyd()
            if m.lloyd[L].w:
                emit(("l_weight", L, 0))
            emit(("l_bind", L, ODD, st()))
            emit(("refuse", what, L, rint(0, 2)))
            emit(("l_assign", L, ODD, st()))                  # still unweighted, still bound
        else:
            L = need_lloyd(hi=64)
            if m.lloyd[L].k > 256:
                emit(("l_re", L, pick_k(hi=64)))
                emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
            if not m.lloyd[L].w:
                make_settable(L)
                emit(("l_weight", L, 1))
            i = pick([ODD, MAP])
            emit(("refuse", what, L, i))
            emit(("l_assign_update", L, i, 1, 1, st()))

    def motif_weight_cutoff():
        """weight on / cutoff 0 -> 128 -> 0 / weight off around the same palette + reduce_indexed + reduce: the first and the last
        results are the default path's; INDEX8 at k = 256 is legal at t = 0 under weighting"""
        emit(("motif", "weight_cutoff"))
        t0, w0 = m.t, m.w
        if m.fid:
            emit(("fixed", 0))
        i, k = pick([ODD, SPRITE]), rint(2, 10)
        at = [("palette", i, k), ("reduce_indexed", i, k, pick([0, 1, 3]), 1), ("reduce", i, k, rint(0, 4))]
        restore_cutoff(0)
        set_weight(0)
        for op in at:
            emit(op)
        emit(("weight", 1))
        for t in (0, 128, 0):
            restore_cutoff(t)
            for op in at:
                emit(op)
        emit(("reduce_indexed", FEW, 256, 0, 0))
        emit(("weight", 0))
        for op in at:
            emit(op)
        restore_cutoff(t0)
        set_weight(w0)

    def motif_weight_adds():
        """two frames added with the switch differing between the adds, the palette taken with the switch both ways"""
        emit(("motif", "weight_adds"))
        S, t0, w0 = rint(0, 2), m.t, m.w
        if m.fid == 3:
            emit(("fixed", 0))
        emit(("s_new", S) if m.seq[S] is None else ("s_clear", S))
        restore_cutoff(0)
        first = rint(0, 2)
        set_weight(first)
        emit(("s_add", S, pick([SPRITE, ODD]), rint(0, 2), st()))
        emit(("weight", 1 - first))
        emit(("s_add", S, pick([4, 1, MAP]), rint(0, 2), st()))
        emit(("s_info", S))
        k = n_fixed_of(m.fid) + rint(2, 8)
        emit(("s_centroids", S, k))
        emit(("weight", first))
        emit(("s_palette", S, k))
        emit(("s_centroids", S, k))
        restore_cutoff(t0)
        set_weight(w0)

    def motif_weight_warm():
        """a warm local output whose frames alternate weighted and unweighted, across a cutoff switch"""
        emit(("motif", "weight_warm"))
        S, t0, w0 = rint(0, 2), m.t, m.w
        fam = pick([0, 1])
        F = LOCAL_FAMILIES[fam]
        open_local(S, fam=fam, k=rint(3, 16), warm=1)
        set_weight(1)
        frame_local(S, F[0])
        emit(("weight", 0))
        frame_local(S, F[1], 1, pick([None, 40]))
        emit(("cutoff", pick([x for x in CUTOFFS if x != m.t])))
        emit(("weight", 1))
        frame_local(S, F[-1])
        emit(("weight", 0))
        frame_local(S, F[0], 1, pick([None, 4096]))
        emit(("weight", 1))
        frame_local(S, F[1])
        restore_cutoff(t0)
        set_weight(w0)

    def motif_weight_binding():
        """an initialisation under the forced colour table leaves its binding; weight 1, run, weight 0, assign_update: the last call
        is unweighted and right.  Then the same with the caller's binding in between, and the setter's refusal"""
        emit(("motif", "weight_binding"))
        L, s0 = rint(0, 2), m.strategy
        if m.strategy != 2:
            emit(("strategy", 2))
        emit(("l_new" if m.lloyd[L] is None else "l_re", L, rint(4, 13)))
        i = pick([ODD, SPRITE, MAP])
        emit(("l_init", L, i, 0, st()))
        emit(("l_weight", L, 1))
        emit(("l_run", L, i, 1, st()))
        emit(("l_weight", L, 0))
        emit(("l_assign_update", L, i, 1, 1, st()))
        emit(("l_init", L, i, pick([0, 1]), st()))
        emit(("l_weight", L, 1))                              # (the binding of the initialisation: dropped by the setter)
        emit(("l_assign", L, i, st()))
        emit(("l_weight", L, 0))
        emit(("l_init", L, i, 0, st()))
        emit(("l_weight", L, 0))                              # (no change: the binding of the initialisation stays)
        emit(("l_assign", L, i, st()))
        emit(("l_bind", L, i, st()))
        emit(("refuse", "l_weight_under_caller_binding", L, 1))
        emit(("l_assign", L, i, st()))
        emit(("refuse", "l_weight_under_caller_binding", L, 0))
        emit(("l_unbind", L))
        emit(("l_weight", L, 1))
        emit(("refuse", "weighted_bind", L, i))
        emit(("l_run", L, i, 1, st()))
        emit(("l_weight", L, 0))
        emit(("l_assign_update", L, i, 1, 1, st()))
        if m.strategy != s0:
            emit(("strategy", s0))

    def motif_weight_blocks():
        """a weighted Lloyd object closed and an unweighted one created in its block, and the reverse, beside host calls under the
        opposite processor weighting: neither the object's nor the library's own object leaks its weighting"""
        emit(("motif", "weight_blocks"))
        w0 = m.w
        for first in (1, 0):
            L = rint(0, 2)
            emit(("l_new" if m.lloyd[L] is None else "l_re", L, rint(3, 40)))
            emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
            emit(("l_weight", L, first))
            emit(("l_assign_update", L, pick([ODD, MAP]), 1, 1, st()))
            set_weight(1 - first)
            emit(("palette", SPRITE, n_fixed_of(m.fid) + rint(2, 8)))
            emit(("l_close", L))
            emit(("l_new", L, rint(3, 40)))
            emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
            if not first:
                emit(("l_weight", L, 1))
            emit(("l_assign_update", L, pick([ODD, MAP]), 1, 1, st()))
            emit(("reduce_indexed", pick([SPRITE, MAP]), n_fixed_of(m.fid) + rint(2, 8), 0, 0))
        set_weight(w0)

    def motif_weight_fixed():
        """fixed colours and weighting: a pinned entry stays put whatever its members weigh and counts as converged; a free cluster
        of total weight 0 is an empty cluster"""
        emit(("motif", "weight_fixed"))
        w0 = m.w
        emit(("fixed", pick([2, 3])))
        f = n_fixed_of(m.fid)
        set_weight(1)
        emit(("palette", SPRITE, f + rint(1, 5)))
        if m.n_kept(ROW, m.wc()):
            emit(("reduce_indexed", ROW, f + rint(1, 4), 0, 0))
        L = rint(0, 2)
        emit(("l_new" if m.lloyd[L] is None else "l_re", L, rint(40, 80)))
        emit(("l_init", L, ROW, 3, st()))
        emit(("l_fix", L, 3))
        emit(("l_weight", L, 1))
        emit(("l_assign_update", L, ROW, 1, 1, st()))
        emit(("l_conv", L, st()))
        emit(("l_run", L, COL, 1, st()))
        emit(("l_iterate", L, ROW, 2, st()))
        emit(("l_conv", L, st()))
        emit(("fixed", 0))
        set_weight(w0)

    def motif_weight_quality():
        """the quality search with weighting on, then off, on the sprite: both records unweighted, the palettes differ"""
        emit(("motif", "weight_quality"))
        w0 = m.w
        if m.fid:
            emit(("fixed", 0))
        args = (SPRITE, pick([4.0, 9.0]), 2, 12, pick([0, 1, 3]), rint(0, 2), 0)
        set_weight(1)
        emit(("quality",) + args)
        emit(("weight", 0))
        emit(("quality",) + args)
        set_weight(w0)

    # ---- surface 4: the batched calls -----------------------------------------------------------------------------------------
    def shape_of(i):
        return images[i][1].shape[:2]

    def batch_list(pool, n=None):
        """image indices drawn with replacement (an image may appear twice), in a random order: lengths 1, 2 and 3 .. 9"""
        if n is None:
            c = rng.random()
            n = 1 if c < 0.15 else 2 if c < 0.35 else rint(3, 10)
        return tuple(pick(list(pool)) for _ in range(n))

    def kept_pool():
        return [i for i in BATCH_POOL if m.n_kept(i, m.t) > 0]

    def swap(imgs, old, new):
        return tuple(new if i == old else i for i in imgs)

    def pairs_bound(call, imgs, fmt):
        """the bytes two neighbours keep resident, where that bound cuts the list after every second image; else None"""
        sizes = [batch_resident(shape_of(i), m.t, call, fmt) for i in imgs]
        B = max(sum(sizes[j:j + 2]) for j in range(0, len(sizes), 2))
        return B if [len(p) for p in batch_cut(sizes, B)] == [2] * (len(imgs) // 2) + [1] * (len(imgs) % 2) else None

    def batch_bound(call, imgs, fmt, pool):
        """(images, max_resident_bytes): 0; 1, a sub-batch per image; or a bound that cuts after every second image -- where the
        drawn list has none, images of one size (a family) take its place"""
        c = rint(0, 3)
        if c < 2:
            return imgs, c
        B = pairs_bound(call, imgs, fmt)
        if B is None:
            fam = pick([f for f in FAMILIES if all(i in pool for i in f)])
            imgs = tuple(pick(list(fam)) for _ in imgs)
            B = pairs_bound(call, imgs, fmt)
        assert B is not None, (call, imgs, fmt)                   # (images of one size keep the same bytes: two fit, three do not)
        return imgs, B

    def batch_k(imgs, fmt=0):
        cap = min(cap_k(min(m.n_kept(i, m.t), 65536)) for i in imgs)
        return pick_k(hi=min(cap, 255 + (0 if m.t else 1) if fmt == 1 else 512))

    def plain_switches(refuse=True):
        """the three calls with a palette step refuse fixed colours and weighting: both off, now and then after the refusal"""
        if m.fid:
            if refuse and rng.random() < 0.4:
                emit(("refuse", "batch_fixed", pick(list(BATCH_PALETTE_CALLS)), batch_list(kept_pool(), rint(1, 4)), rint(8, 20)))
            emit(("fixed", 0))
        if m.w:
            if refuse and rng.random() < 0.4:
                emit(("refuse", "batch_weighted", pick(list(BATCH_PALETTE_CALLS)), batch_list(kept_pool(), rint(1, 4)), rint(2, 20)))
            emit(("weight", 0))

    def output_args(fmt=None, mode=None):
        fmt = pick([0, 1, 2]) if fmt is None else fmt
        if mode is None:
            mode = pick([0, 0, 1, 1, 3]) if fmt else pick([0, 0, 1, 1, 2, 3])
        return fmt, mode

    def small_enough(imgs, mode, k, output_step=True):
        """no diffusion of the 300 x 200 image (the reference's is a Python loop), and in a batched output step no dither of it with
        128 colours or more (include/kmeans_hip.h leaves whether it joins the launch to a measured rule)"""
        if mode == 3 or (output_step and mode == 1 and k >= 128):
            return swap(imgs, BIG, ODD)
        return imgs

    def host_batch(call, imgs=None, k=None, algo=0, mode=None, fmt=None, bound=None):
        plain_switches()
        pool = kept_pool()
        imgs = batch_list(pool) if imgs is None else imgs
        if call == "b_palette":
            fmt, mode = 0, 0
        else:
            fmt, mode = output_args(0 if call == "b_reduce" else fmt, mode)
        k = batch_k(imgs, fmt) if k is None else k
        imgs = small_enough(imgs, mode, k, call == "b_reduce_indexed")
        if bound is None:
            imgs, bound = batch_bound(call, imgs, fmt, pool)
        emit({"b_palette": ("b_palette", imgs, k, algo, bound), "b_reduce": ("b_reduce", imgs, k, algo, mode, bound),
              "b_reduce_indexed": ("b_reduce_indexed", imgs, k, algo, mode, fmt, bound)}[call])

    def find_batch(imgs=None, k=None, mode=None, fmt=None, bound=None):
        pool = list(BATCH_POOL) + [CLEAR]
        imgs = batch_list(pool) if imgs is None else imgs
        fmt, mode = output_args(fmt, mode)
        k = pick_k(hi=255 + (0 if m.t else 1) if fmt == 1 else 300) if k is None else k
        imgs = small_enough(imgs, mode, k)
        if bound is None:
            imgs, bound = batch_bound("b_find", imgs, fmt, pool)
        emit(("b_find", imgs, k, rint(0, 1 << 30), mode, fmt, bound))

    def palette_device(imgs=None, k=None):
        imgs = batch_list(list(BATCH_POOL) + [CLEAR]) if imgs is None else imgs
        n = max(shape_of(i)[0] * shape_of(i)[1] for i in imgs)
        emit(("b_palette_device", imgs, pick_k(hi=512 if n <= 8000 else 256) if k is None else k))

    def apply_device(imgs=None, k=None, shared=None, mode=None, fmt=None):
        imgs = batch_list(list(BATCH_POOL) + [CLEAR]) if imgs is None else imgs
        fmt, mode = output_args(fmt, mode)
        k = pick_k(hi=255 + (0 if m.t else 1) if fmt == 1 else 400) if k is None else k
        imgs = small_enough(imgs, mode, k)
        emit(("b_apply_device", imgs, k, rint(0, 1 << 30), rint(0, 2) if shared is None else shared, mode, fmt, pick(list(CPAIR_OFFSETS))))

    def family_pairs():
        """five to nine images of one size at the bound of two of them, in a call with a palette step and in the find call: the
        list is cut after every second image, three or four times"""
        fam = pick([f for f in FAMILIES if all(m.n_kept(i, m.t) > 0 for i in f)])
        imgs = tuple(pick(list(fam)) for _ in range(rint(5, 10)))
        call, mode, k = pick(list(BATCH_PALETTE_CALLS)), pick([0, 1]), rint(2, 40)
        fmt = 1 if call == "b_reduce_indexed" else 0
        host_batch(call, imgs, k, mode=mode, fmt=fmt, bound=pairs_bound(call, imgs, fmt))
        fmt = pick([0, 1, 2])
        find_batch(imgs, k, mode, fmt, pairs_bound("b_find", imgs, fmt))

    def batch_ops():
        c = rng.random()
        if c < 0.6:
            host_batch(pick(list(BATCH_PALETTE_CALLS)))
        elif c < 0.75:
            find_batch()
        elif c < 0.87:
            palette_device()
        else:
            apply_device()

    def refusal_4(what):
        small = [i for i in (ODD, SPRITE, FEW, FLAT, ROW, MAP) if m.n_kept(i, m.t) > 0]
        if what in ("batch_fixed", "batch_weighted"):
            call, imgs, k = pick(list(BATCH_PALETTE_CALLS)), batch_list(small, rint(1, 5)), rint(8, 20)
            if what == "batch_fixed" and not m.fid:
                emit(("fixed", pick([1, 2, 3])))
            if what == "batch_weighted":
                if m.fid:
                    emit(("fixed", 0))
                set_weight(1)
            emit(("refuse", what, call, imgs, k))
            plain_switches(refuse=False)
            host_batch(call, imgs, k, bound=pick([0, 1]))
        elif what == "batch_no_kept_pixel":
            t0 = m.t
            plain_switches(refuse=False)
            if m.t == 0:
                emit(("cutoff", pick([1, 128, 255])))
            call, k = pick(list(BATCH_PALETTE_CALLS)), rint(2, 12)
            imgs = list(batch_list([i for i in (ODD, SPRITE, FEW, FLAT, MAP) if m.n_kept(i, m.t) > 0], rint(1, 5)))
            imgs.insert(rint(0, len(imgs) + 1), CLEAR)
            emit(("refuse", what, call, tuple(imgs), k, pick([0, 1])))
            host_batch(call, tuple(i for i in imgs if i != CLEAR), k, bound=1)
            restore_cutoff(t0)
        elif what in ("batch_index8_full", "batch_meld_indexed"):
            call, imgs = pick(["b_find", "b_reduce_indexed", "b_apply_device"]), batch_list(small, rint(1, 4))
            if what == "batch_index8_full":
                k = 256 if m.t else 257
                emit(("refuse", what, call, imgs, k))
                good = dict(k=k - 1, mode=0, fmt=1)
            else:
                emit(("refuse", what, call, imgs, 5, pick([1, 2])))
                good = dict(k=5, mode=2, fmt=0)
            if call == "b_find":
                find_batch(imgs, bound=0, **good)
            elif call == "b_apply_device":
                apply_device(imgs, **good)
            else:
                plain_switches(refuse=False)
                host_batch(call, imgs, bound=0, **good)
        elif what == "batch_bad_tables":
            imgs = batch_list(small, rint(3, 6))
            emit(("refuse", what, imgs, rint(2, 40), pick([0, 2, len(imgs) + 1])))
            apply_device(imgs, shared=0)
        else:
            assert what == "batch_empty", what
            emit(("refuse", what, pick(list(BATCH_OPS))))

    def motif_batch_shrinking():
        """nine images at k = 300, two others at k = 3, one at k = 33, through the host call, the indexed call and the device call:
        n, k and the sizes shrink, so every word a recycled block still holds differs from the one the next batch needs"""
        emit(("motif", "batch_shrinking"))
        t0 = m.t
        plain_switches(refuse=False)
        nine = (ODD, 1, SPRITE, 3, 4, FEW, FLAT, ROW, COL)
        if not all(m.n_kept(i, m.t) for i in nine + (11, 13)):
            restore_cutoff(0)
        nine = tuple(nine[int(j)] for j in rng.permutation(9))
        steps = ((nine, 300), (pick([(11, 13), (MAP, BIG), (13, MAP)]), 3), ((pick([ODD, MAP, FEW]),), 33))
        for imgs, k in steps:
            emit(("b_palette", imgs, k, 0, 0))
        mode = pick([0, 1])
        for imgs, k in steps:
            emit(("b_reduce_indexed", imgs, k, 0, mode, 2 if k > 255 else 1, 0))
        for imgs, k in steps:
            emit(("b_palette_device", imgs, k))
        family_pairs()
        restore_cutoff(t0)

    def motif_batch_device_blocks():
        """kmg_dev_palette_batch twice with different images, a Lloyd object created, run and closed in the block between them"""
        emit(("motif", "batch_device_blocks"))
        L = rint(0, 2)
        palette_device((SPRITE, FEW, ODD, FLAT, MAP)[:rint(3, 6)], rint(4, 40))
        if m.lloyd[L] is not None:
            emit(("l_close", L))
        emit(("l_new", L, pick_k(hi=64)))
        emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
        emit(("l_run", L, FEW, 1, st()))
        emit(("l_close", L))
        palette_device((COL, 1, FEW)[:rint(2, 4)], rint(2, 12))

    def motif_batch_cutoff():
        """cutoff 0 -> 128 -> 0 around the indexed call and the find call, then the device output call at each cutoff with one
        shared and one table per image: every batched call reads the cutoff when it starts"""
        emit(("motif", "batch_cutoff"))
        t0 = m.t
        plain_switches(refuse=False)
        imgs, k, seed = batch_list([SPRITE, ODD, 3, ROW, MAP, 1], rint(2, 6)), rint(3, 40), rint(0, 1 << 30)
        mode, bound = pick([0, 1]), pick([0, 1])
        for t in (0, 128, 0):
            restore_cutoff(t)
            emit(("b_reduce_indexed", imgs, k, 0, mode, pick([1, 2]), bound))
            emit(("b_find", imgs + (CLEAR,), k, seed, mode, 1, bound))
        for t in (128, 0):
            restore_cutoff(t)
            emit(("b_apply_device", imgs, k, seed, 1, mode, pick([1, 2]), pick(list(CPAIR_OFFSETS))))
            emit(("b_apply_device", imgs, k, seed, 0, pick([0, 1, 3]), 0, pick(list(CPAIR_OFFSETS))))
        restore_cutoff(t0)

    def motif_batch_switches():
        """fixed colours on: the find call works and equals the unpinned model, the three calls with a palette step refuse; off: the
        same calls work.  Then the same with alpha weighting"""
        emit(("motif", "batch_switches"))
        w0 = m.w
        imgs = batch_list([i for i in (ODD, SPRITE, FEW, MAP, ROW) if m.n_kept(i, m.t) > 0], rint(2, 5))
        k, seed, mode = rint(8, 24), rint(0, 1 << 30), pick([0, 1])
        calls = [("b_reduce_indexed", imgs, k, 0, mode, 1, 0), ("b_palette", imgs, k, 0, 0), ("b_reduce", imgs, k, 0, mode, pick([0, 1]))]
        set_weight(0)
        for what in ("batch_fixed", "batch_weighted"):
            if what == "batch_fixed":
                emit(("fixed", pick([1, 2, 3])))
            else:
                emit(("weight", 1))
            emit(("b_find", imgs, k, seed, mode, 1, 0))
            for op in calls:
                emit(("refuse", what, op[0], imgs, k))
            emit(("fixed", 0) if what == "batch_fixed" else ("weight", 0))
            emit(("b_find", imgs, k, seed, mode, 1, 0))
            for op in calls:
                emit(op)
        set_weight(w0)

    def motif_batch_no_kept_pixel():
        """the image without a kept pixel last in the list, at bound 0 and at bound 1 (the up-front pass); then the same list without
        it at bound 1 and at bound 0, in the blocks the refused calls gave back"""
        emit(("motif", "batch_no_kept_pixel"))
        t0 = m.t
        plain_switches(refuse=False)
        if m.t == 0:
            emit(("cutoff", pick([1, 128, 255])))
        imgs = batch_list([i for i in (ODD, SPRITE, FEW, FLAT, MAP) if m.n_kept(i, m.t) > 0], rint(2, 5))
        call, k = pick(list(BATCH_PALETTE_CALLS)), rint(2, 12)
        for bound in (0, 1):
            emit(("refuse", "batch_no_kept_pixel", call, imgs + (CLEAR,), k, bound))
        for bound in (1, 0):
            host_batch(call, imgs, k, mode=pick([0, 1]), fmt=1 if call == "b_reduce_indexed" else 0, bound=bound)
        restore_cutoff(t0)

    def motif_batch_beside_objects():
        """batched calls between the frames of an open output and beside a bound Lloyd object: the next frame and the next assign
        are still right"""
        emit(("motif", "batch_beside_objects"))
        S, L = rint(0, 2), rint(0, 2)
        plain_switches(refuse=False)
        small_sequence(S)
        emit(("s_output", S, rint(2, 30), pick([0, 1, 3]), 1, 1))
        emit(("s_frame", S, SPRITE, 1, None))
        emit(("l_new" if m.lloyd[L] is None else "l_re", L, rint(4, 13)))
        emit(("l_set", L, "rand", rint(0, 1 << 30), ODD))
        emit(("l_bind", L, ODD, st()))
        emit(("l_assign", L, ODD, st()))
        host_batch("b_reduce_indexed", bound=0)
        emit(("s_frame", S, 3, 1, pick([None, 40])))
        emit(("l_assign", L, ODD, st()))
        palette_device()
        apply_device()
        emit(("s_frame", S, 4, 1, None))
        emit(("l_assign_update", L, ODD, 1, 1, st()))

    def motif_batch_octree():
        """octree batches (the host algorithm per image, no batched launch) alternate with k-means batches"""
        emit(("motif", "batch_octree"))
        t0 = m.t
        plain_switches(refuse=False)
        restore_cutoff(0)
        imgs, k = batch_list([SPRITE, 3, 4, FEW, ROW, 11, COL, 13], rint(2, 6)), rint(2, 40)   # (the noise images cost the reference seconds each)
        for algo in (1, 0, 1):
            emit(("b_palette", imgs, k, algo, pick([0, 1])))
            emit(("b_reduce", imgs, k, 1 - algo, pick([0, 1]), 0))
        family_pairs()
        restore_cutoff(t0)

    older = 0.3       # surface 4: fewer of the older passages in a sequence, so that a seed costs what the other surfaces' seeds cost
    motifs = [mo for mo in (motif_mixed, motif_refusals, motif_cutoff, motif_reoutput, motif_anchor, motif_growth, motif_first_frame, motif_freeze, motif_pins) if rng.random() < (0.75 if surface < 4 else older)]
    if surface >= 2:
        motifs += [mo for mo in (motif_warm_cutoff, motif_refused_warm, motif_used_block, motif_lossy_full, motif_local_shared_local,
                                 motif_optimize_path, motif_records, motif_cpair) if rng.random() < (0.8 if surface < 4 else older)]
    if surface >= 3:
        motifs += [mo for mo in (motif_weight_cutoff, motif_weight_adds, motif_weight_warm, motif_weight_binding, motif_weight_blocks,
                                 motif_weight_fixed, motif_weight_quality) if rng.random() < (0.8 if surface < 4 else older)]
    if surface >= 4:
        motifs += [mo for mo in (motif_batch_shrinking, motif_batch_device_blocks, motif_batch_cutoff, motif_batch_switches,
                                 motif_batch_no_kept_pixel, motif_batch_beside_objects, motif_batch_octree) if rng.random() < 0.8]
    at = sorted(rint(3, n_ops - 5) for _ in motifs)
    motifs = [motifs[int(j)] for j in rng.permutation(len(motifs))]
    emit(("strategy", pick([2, 0, 1], [0.5, 0.3, 0.2])))
    while len(ops) < n_ops or motifs:
        if motifs and len(ops) >= at[0]:
            at.pop(0)
            motifs.pop(0)()
            continue
        if surface >= 4 and rng.random() < 0.45:
            batch_ops()
            continue
        if surface >= 2 and rng.random() < 0.4:
            surface_2_ops()
            continue
        r = rng.random()
        if r < 0.1:
            switches()
        elif r < 0.27:
            host()
        elif r < 0.52:
            device()
        elif r < 0.74:
            lloyd_ops()
        elif r < 0.96:
            sequence_ops()
        else:
            refusal()
    for L in range(2):
        if m.lloyd[L] is not None:
            emit(("l_close", L))
    for S in range(2):
        if m.seq[S] is not None:
            emit(("s_close", S))
    if m.w:
        emit(("weight", 0))
    return ops


# ---- one op on the model ----------------------------------------------------------------------------------------------
def apply_op(m, op):
    """advances the model by `op`; numeric: returns what the runner compares"""
    name, num, R = op[0], m.numeric, m.ref
    exp = {}
    if name == "cutoff":
        m.t = op[1]
    elif name == "fixed":
        m.fid = op[1]
    elif name == "strategy":
        m.strategy = op[1]
    elif name == "weight":
        assert op[1] in (0, 1), op
        m.w = op[1]
    elif name == "motif":
        assert op[1] in MOTIFS_3 + MOTIFS_4, op
    elif name in BATCH_OPS:
        apply_op_4(m, op, exp)
    elif name in ("palette", "reduce", "reduce_indexed"):
        i, k = op[1], op[2]
        assert k >= n_fixed_of(m.fid) and m.n_kept(i, m.wc()) > 0, op
        if num:
            cent = R.centroids(((i, m.wc()),), k, m.fid, m.w)               # (the outputs below: their cutoff stays t)
            if name == "palette":
                exp["palette"] = sorted_palette(cent)
            elif name == "reduce":
                exp["image"] = R.rgba(R.img(i), cent, op[3], m.t)
            else:
                exp["palette"] = R.palette_bytes(cent)
                exp["index"] = R.index(R.img(i), cent, op[3], m.t)
                exp["image"] = R.rgba(R.img(i), cent, op[3], m.t)
    elif name in ("find", "find_indexed"):
        i, k, mode, seed = op[1:5]
        if num:
            pal = find_palette(seed, k)
            if name == "find":
                exp["image"] = (alpha_ref.find(O, R.img(i), pal, mode, m.t) if m.t else
                                diffuse_ref.diffuse(R.img(i), diffuse_ref.oracle_find_replace(O, pal)) if mode == 3 else O.find(R.img(i), pal, mode))
            else:
                exp["index"] = R.index(R.img(i), R.find_centroids(pal), mode, m.t)
    elif name == "quality":
        i, dE, k_min, k_max, mode, indexed = op[1:7]
        assert k_min >= n_fixed_of(m.fid), op
        if num:
            k, reached, rec = R.quality(i, m.wc(), m.fid, target_of(dE), k_min, k_max, m.w)
            cent = R.centroids(((i, m.wc()),), k, m.fid, m.w)
            exp.update(k=k, reached=reached, stats=rec, palette=R.palette_bytes(cent))
            exp["out"] = R.index(R.img(i), cent, mode, m.t) if indexed else R.rgba(R.img(i), cent, mode, m.t)
    elif name in ("apply", "apply_plan"):
        i, mode, fmt, k, seed = op[1:6]
        assert fmt != 1 or k + (1 if m.t else 0) <= 256, op
        if num:
            cent, _ = gamut_centroids(seed, k)
            exp["cent"] = cent
            exp["out"] = R.rgba(R.img(i), cent, mode, m.t) if fmt is None else R.index(R.img(i), cent, mode, m.t)
        if name == "apply_plan":
            m.t = op[6]
    elif name == "compact":
        if num:
            exp["kept"] = alpha_ref.compact(R.img(op[1]), op[2])
    elif name == "compare_device":
        i, other, fmt, k, seed, nb, order, cut, what, fresh = op[1:11]
        if num:
            cent, _ = gamut_centroids(seed, k)
            src = R.img(i)
            exp["cent"] = cent
            exp["out"] = R.rgba(src, cent, 0, m.t) if fmt is None else R.index(src, cent, 0, m.t)
            exp["palette"] = None if fmt is None else R.palette_bytes(cent)
            if fresh:
                m.rec = error_ref.ZERO
            m.rec = error_ref.combine(m.rec, R.stats(src, exp["out"], exp["palette"], cut, what))
            exp["record"] = m.rec
    elif name == "pair_open":
        P, fam, fmt, k, seed, mode = op[1:7]
        assert fmt != 1 or k <= 255, op
        h, w = m.images[FAMILIES[fam][0]][1].shape[:2]
        m.pairs[P] = dict(fam=fam, fmt=fmt, k=k, seed=seed, mode=mode, canvas=np.full((h, w), k, np.int64), held=np.zeros((h, w, 4), np.uint8),
                          last=None)
    elif name == "pair_frame":
        P, i, tol = op[1:4]
        pr = m.pairs[P]
        assert pr is not None and i in FAMILIES[pr["fam"]], op
        if num:
            cent, _ = gamut_centroids(pr["seed"], pr["k"])
            src = R.img(i)
            I = R.index(src, cent, pr["mode"], m.t)
            exp.update(cent=cent, index=I)
            if tol is None:
                d, pr["canvas"], rec = R.delta(I, pr["canvas"], pr["k"])
                pr["held"] = src.copy()                              # (the caller's duty after an exact frame)
                rec = tuple(rec) + (0, 0)
            else:
                d, pr["canvas"], pr["held"], rec = R.hold(src, I, pr["canvas"], pr["held"], pr["k"], tol)
            exp.update(delta=d, canvas=pr["canvas"], held=pr["held"], record=tuple(rec))
        pr["last"] = "exact" if tol is None else "lossy"
    elif name in ("l_new", "l_re"):
        m.lloyd[op[1]] = LSlot(op[2])                         # (unweighted and unbound, whatever its block's last owner was)
        if num:
            m.lloyd[op[1]].acc = np.zeros((op[2], 4), np.int64)
    elif name == "l_close":
        m.lloyd[op[1]] = None
    elif name.startswith("l_"):
        s = m.lloyd[op[1]]
        assert s is not None, op
        if name in LLOYD_IMAGE_OPS and s.bind is not None and s.bind != op[2]:
            exp["unbind"] = True                              # (whether a pass on other pixels re-binds is the cost model's)
            s.bind = s.owner = None
        if name == "l_set":
            s.cent = make_centroids(op[2], op[3], s.k, m.images[op[4]][1]) if num else True
        elif name == "l_init":
            i, f = op[2], op[3]
            assert f <= s.k
            h, w = m.images[i][1].shape[:2]
            forced = {0: 0, 1: -1, 2: 1}[m.strategy]
            s.bind = None if (s.k == 1 or forced < 0) else i
            s.owner = "init" if forced > 0 and s.k > 1 else "unsure" if s.owner in ("caller", "unsure") else None
            s.nconv = None
            s.cent = R.seeded(i, s.k, f) if num else True
            exp["cent"] = s.cent
        elif name == "l_fix":
            assert op[2] <= s.k
            s.f = op[2]
        elif name == "l_bind":
            assert not s.w, op
            s.bind, s.owner = op[2], "caller"
        elif name == "l_unbind":
            s.bind = s.owner = None
        elif name == "l_weight":
            assert op[2] in (0, 1) and s.owner in (None, "init"), op
            exp["owner"] = s.owner
            if op[2] != s.w:                                  # a binding the initialisation left ends here, in both directions
                s.bind = s.owner = None
            s.w = op[2]
        elif name == "l_conv":
            assert s.nconv is not None
            exp["nconv"] = s.nconv
        else:
            assert s.cent is not None, op
            if name == "l_update":
                if num:
                    lloyd_step(s, s.acc)
                    exp["cent"] = s.cent
                else:
                    s.nconv = True
            elif name == "l_assign":
                if num:
                    exp["cent_before"] = s.cent
                    exp["labels"], s.acc = R.assign(op[2], s.cent, s.w)
            elif name == "l_assign_update":
                if num:
                    exp["cent_before"] = s.cent
                    labels, s.acc = R.assign(op[2], s.cent, s.w)
                    if op[3]:
                        exp["labels"] = labels
                    if op[4]:
                        lloyd_step(s, s.acc)
                    exp["cent"] = s.cent
                elif op[4]:
                    s.nconv = True
            elif name == "l_iterate":
                if num:
                    for _ in range(op[3]):
                        lloyd_step(s, s.acc)
                        labels, s.acc = R.assign(op[2], s.cent, s.w)
                    exp.update(labels=labels, cent=s.cent)
                s.nconv = s.nconv if num else True
            elif name == "l_run":
                if num:
                    s.cent, labels, it = R.run(op[2], s.cent, s.f, s.w)
                    exp.update(cent=s.cent, iterations=it)
                    if op[3]:
                        exp["labels"] = labels
                s.nconv = None
                # a caller's binding of these pixels is trusted and stays; any other one is (re)made and dropped by the run
                s.owner = "caller" if s.owner == "caller" and s.bind == op[2] else "unsure" if s.owner in ("caller", "unsure") else None
                s.bind = None
            elif name == "l_lftu":
                assert s.k <= 256 and not s.w, op
                s.bind, s.owner = op[2], "caller"
                if num:
                    exp["labels"], sums = R.assign(op[2], s.cent)
                    lloyd_step(s, sums)
                    s.acc = np.zeros_like(s.acc)
                    exp["cent"] = s.cent
                else:
                    s.nconv = True
            else:
                raise ValueError(op)
    elif name == "s_new":
        assert m.seq[op[1]] is None
        m.seq[op[1]] = SSlot()
    elif name == "s_close":
        m.seq[op[1]] = None
    elif name.startswith("s_"):
        q = m.seq[op[1]]
        assert q is not None, op
        if name == "s_add":
            q.frames.append((op[2], m.wc()))
            q.wadd.append(m.w)
        elif name == "s_clear":
            q.frames, q.wadd = [], []
        elif name == "s_info":
            if num:
                exp["info"] = (len(q.frames), sum(R.kept(i, t)[0].shape[0] for i, t in q.frames))
        elif name in ("s_centroids", "s_palette"):
            assert op[2] >= n_fixed_of(m.fid) and m.seq_pixels(op[1]) > 0, op
            if num:
                cent = R.centroids(m.frames_of(op[1]), op[2], m.fid, m.w)
                exp["cent" if name == "s_centroids" else "palette"] = cent if name == "s_centroids" else sorted_palette(cent)
        elif name == "s_output":
            k, mode, fmt, fam = op[2:6]
            assert k >= n_fixed_of(m.fid) and m.seq_pixels(op[1]) > 0 and (fmt != 1 or k <= 255) and (fmt == 0 or mode != 2), op
            h, w = m.images[FAMILIES[fam][0]][1].shape[:2]
            q.out = dict(t=m.t, k=k, mode=mode, fmt=fmt, fam=fam, cent=None, canvas=np.full((h, w), k, np.int64), held=np.zeros((h, w, 4), np.uint8),
                         last=None, shape=(h, w), coded=[])
            if num:
                q.out["cent"] = R.centroids(m.frames_of(op[1]), k, m.fid, m.w)
                exp["palette"] = R.palette_bytes(q.out["cent"])
        elif name == "s_end":
            q.out = None
        elif name == "s_frame":
            i, delta, tol = op[2:5]
            o = q.out
            assert o is not None and not o.get("local") and i in FAMILIES[o["fam"]] and (o["fmt"] != 0 or (not delta and tol is None)) and \
                (tol is None or delta), op
            if o["fmt"] and not num:
                o["coded"].append(None)
            kind = "exact" if tol is None else "lossy"
            exp["transition"] = None if o["last"] in (None, kind) else o["last"] + ">" + kind
            o["last"] = kind
            if num:
                src = R.img(i)
                if o["fmt"] == 0:
                    exp.update(map=R.rgba(src, o["cent"], o["mode"], o["t"]), record=sequence_ref.FRESH, full=True)
                    return exp
                I = R.index(src, o["cent"], o["mode"], o["t"])
                if tol is None:
                    d, canvas, rec = R.delta(I, o["canvas"], o["k"])
                    held = src.copy()
                    full = (not delta) or rec[1] > 0
                    if not delta:
                        rec = sequence_ref.FRESH
                else:
                    d, canvas, held, rec = R.hold(src, I, o["canvas"], o["held"], o["k"], tol)
                    full = rec[1] > 0
                    if full:
                        canvas, held = I.copy(), src.copy()
                o["canvas"], o["held"] = canvas, held
                exp.update(map=I if full else d, record=tuple(rec), full=full, fallback=bool(delta and full))
                o["coded"].append((exp["map"], None, full))
        elif name == "s_output_local":
            k, mode, fmt, fam, warm = op[2:7]
            assert fmt in (1, 2) and (fmt != 1 or k <= 255) and mode in (0, 1, 3), op
            h, w = m.images[LOCAL_FAMILIES[fam][0]][1].shape[:2]
            q.out = dict(local=True, k=k, mode=mode, fmt=fmt, fam=fam, warm=warm, shape=(h, w), prev=None, failed=None, last=None, coded=[],
                         shown=np.zeros((h, w), np.uint32), held=np.zeros((h, w, 4), np.uint8))
        elif name == "s_frame_local":
            exp.update(local_frame(m, q.out, op[2], op[3], op[4]))
        elif name in ("s_usage", "s_remap"):
            o = q.out
            assert o is not None and o["coded"] and 0 <= op[4] < len(o["coded"]), op
            k = o["k"]
            if name == "s_usage":
                rec, fresh = op[2], op[3]
                assert fresh or (m.urec[rec] is not None and m.urec[rec]["k"] == k), op
                if num:
                    I, pal, _ = o["coded"][op[4]]
                    old = np.zeros(k + 2, np.uint64) if fresh else m.urec[rec]["counts"]
                    m.urec[rec] = dict(k=k, counts=old + index_ref.usage(I, k), palette=R.palette_bytes(o["cent"]) if pal is None else pal)
                    exp["counts"] = m.urec[rec]["counts"]
                else:
                    m.urec[rec] = dict(k=k)
            else:
                tb = m.tables[op[2]]
                assert tb is not None and tb["k"] == k and op[3] in BITS, op
                if num:
                    new, bad = index_ref.remap_fast(o["coded"][op[4]][0], k, tb["remap"], op[3])
                    exp.update(out=index_ref.pack_fast(new, op[3]), bad=bad, new=new)
        else:
            raise ValueError(op)
    elif name in ("cpair_open", "cpair_frame", "usage_device", "plan", "remap_device", "optimize"):
        apply_op_2(m, op, exp)
    elif name == "refuse":
        exp["status"] = ERR_INVALID
        what = op[1]
        if what in REFUSALS_2:
            refuse_2(m, op, exp)
        if what in REFUSALS_3:
            refuse_3(m, op, exp)
        if what in REFUSALS_4:
            refuse_4(m, op, exp)
        if what in ("k_below_fixed_palette", "k_below_fixed_reduce", "k_below_fixed_sequence"):
            assert op[3] < n_fixed_of(m.fid), op
        elif what == "octree_fixed":
            assert n_fixed_of(m.fid) > 0, op
        elif what == "frame_no_output":
            assert m.seq[op[2]].out is None, op
        elif what in ("delta_on_rgba8", "lossy_on_rgba8"):
            assert m.seq[op[2]].out["fmt"] == 0, op
        elif what == "lossy_without_delta":
            assert m.seq[op[2]].out["fmt"] != 0, op
        elif what == "index8_full":
            assert op[3] + (1 if m.t else 0) == 257, op
        elif what == "empty_sequence":
            assert m.seq_pixels(op[2]) == 0 and m.seq[op[2]].frames, op
    else:
        raise ValueError(op)
    return exp


# ---- surface 2 on the model -------------------------------------------------------------------------------------------
def local_frame(m, o, i, delta, tol):
    """kmg_sequence_output_frame_local on the open local output o: cutoff and fixed colours as they are at THIS call.  A call
    refused before any work is enqueued (fixed colours on a warm output, k below the fixed colours) changes nothing, not even
    whether the next frame is warm; a frame that fails in its palette step leaves shown and held and makes the next frame cold"""
    assert o is not None and o.get("local") and i in LOCAL_FAMILIES[o["fam"]] and (tol is None or delta), (i, delta, tol)
    R, k, f = m.ref, o["k"], n_fixed_of(m.fid)
    wc = m.wc()                                               # (the weighting, as the cutoff, is read at THIS call: cold and warm)
    kind = "fixed_on_warm" if o["warm"] and f else "k_below_fixed" if k < f else "empty" if m.n_kept(i, wc) == 0 else None
    exp = {"after": o["failed"], "failed": kind}
    o["failed"] = kind
    if kind:
        exp["status"] = ERR_UNSUPPORTED if kind == "fixed_on_warm" else ERR_INVALID
        if kind == "empty":
            o["prev"] = None
        return exp
    exp["warm"] = bool(o["warm"] and o["prev"] is not None)
    exp["first_lossy"] = tol is not None and not o["coded"]
    if not m.numeric:
        o["prev"] = True
        o["coded"].append(None)
        return exp
    src = R.img(i)
    cent = R.warm(i, wc, o["prev"], m.w) if exp["warm"] else R.centroids(((i, wc),), k, m.fid, m.w)
    I, P = R.index(src, cent, o["mode"], m.t), R.palette_bytes(cent)
    if not delta:
        d, rec, full = None, local_ref.FRESH8, True
        shown, held = local_ref.lookup(I, P, k)[1], src.copy()
    elif tol is None:
        d, shown, rec = local_ref.colour(I, o["shown"], P, k)
        rec, held, full = tuple(rec) + (0, 0), src.copy(), rec[1] > 0
    else:
        d, shown, held, rec = local_ref.lossy(O, src, I, o["shown"], o["held"], P, k, tol)
        full = rec[1] > 0
        if full:                                              # the viewer then shows P_t[I_t] everywhere
            shown, held = local_ref.lookup(I, P, k)[1], src.copy()
        exp["lossy_full"] = full
    o.update(shown=shown, held=held, prev=cent)
    out = I if full else d
    o["coded"].append((out, P, full))
    exp.update(map=out, palette=P, record=tuple(int(v) for v in rec), full=full, shown=shown, held_pixels=tol is not None and rec[6] > 0)
    return exp


def cpair_palette(pseed, k):
    """(the k colours the map is made for, the palette the canvas is keyed by): in the second some entries repeat an earlier one's
    bytes and one word is zero, as _palette of tests/test_gpu_local.py makes them"""
    base = find_palette(pseed, k)
    pal = base.copy()
    rng = np.random.default_rng([pseed, k, 5])
    if k >= 2:
        for j in rng.integers(1, k, max(1, k // 5)):
            pal[j] = pal[rng.integers(0, j)]
        pal[rng.integers(0, k)] = 0
    return base, np.ascontiguousarray(pal)


def random_table(tseed, k, bits):
    """a remap table nobody planned: new indices that fit, dropped entries, entries too wide for `bits`"""
    rng = np.random.default_rng([tseed, k, bits])
    t = rng.integers(0, min(1 << bits, 0xFFFF), k + 1).astype(np.uint16)
    r = rng.random(k + 1)
    t[r < 0.12] = index_ref.DROPPED
    if bits < 16:
        t[r > 0.92] = (1 << bits) + rng.integers(0, 3)
    return t


def usage_source(m, op):
    """(centroids, index map) of the map usage_device and remap_device make on the device: op[1:6] = image, mode, format, k, seed"""
    i, mode, fmt, k, seed = op[1:6]
    cent, _ = gamut_centroids(seed, k)
    return cent, m.ref.index(m.ref.img(i), cent, mode, m.t)


def apply_op_2(m, op, exp):
    name, num, R = op[0], m.numeric, m.ref
    if name == "cpair_open":
        P, fam, fmt, k, offs = op[1:6]
        assert (fmt != 1 or k <= 255) and offs in CPAIR_OFFSETS, op
        h, w = m.images[FAMILIES[fam][0]][1].shape[:2]
        m.cpairs[P] = dict(fam=fam, fmt=fmt, k=k, offs=offs, pseed=None, shown=np.zeros((h, w), np.uint32), held=np.zeros((h, w, 4), np.uint8))
    elif name == "cpair_frame":
        P, i, pseed, tol = op[1:5]
        pr = m.cpairs[P]
        assert pr is not None and i in FAMILIES[pr["fam"]], op
        pr["pseed"] = pseed
        if num:
            k = pr["k"]
            base, pal = cpair_palette(pseed, k)
            src = R.img(i)
            I = R.index(src, R.find_centroids(base), pseed % 2, m.t)
            if tol is None:
                d, pr["shown"], rec = local_ref.colour(I, pr["shown"], pal, k)
                pr["held"] = src.copy()                              # (the caller's duty after an exact frame)
                rec = tuple(rec) + (0, 0)
            else:
                d, pr["shown"], pr["held"], rec = local_ref.lossy(O, src, I, pr["shown"], pr["held"], pal, k, tol)
            exp.update(base=base, palette=pal, index=I, delta=d, shown=pr["shown"], held=pr["held"], record=tuple(int(v) for v in rec))
    elif name == "usage_device":
        i, mode, fmt, k, seed, rec = op[1:7]
        fresh = op[10]
        assert (fmt != 1 or k + (1 if m.t else 0) <= 256) and (fresh or (m.urec[rec] is not None and m.urec[rec]["k"] == k)), op
        if num:
            cent, I = usage_source(m, op)
            old = np.zeros(k + 2, np.uint64) if fresh else m.urec[rec]["counts"]
            m.urec[rec] = dict(k=k, counts=old + index_ref.usage(I, k), palette=R.palette_bytes(cent))
            exp.update(cent=cent, index=I, counts=m.urec[rec]["counts"])
        else:
            m.urec[rec] = dict(k=k)
    elif name == "plan":
        rec, slot, flags = op[1:4]
        u = m.urec[rec]
        assert u is not None and (flags & 3) != 3 and not flags & ~index_ref.ALL_FLAGS, op
        if num:
            remap, pal, info = index_ref.plan(u["counts"], u["palette"], flags)         # (a record of maps counted here is never empty)
            m.tables[slot] = dict(k=u["k"], remap=remap, palette=pal, info=info)
            exp.update(counts=u["counts"], source=u["palette"], remap=remap, palette=pal, info=info)
        else:
            m.tables[slot] = dict(k=u["k"])
    elif name == "remap_device":
        i, mode, fmt, k, seed, table, bits, in_place, bad_fresh = op[1:10]
        assert (fmt != 1 or k + (1 if m.t else 0) <= 256) and bits in BITS and (not in_place or bits == 8 * fmt), op
        assert not isinstance(table, int) or (m.tables[table] is not None and m.tables[table]["k"] == k), op
        if num:
            cent, I = usage_source(m, op)
            tb = m.tables[table]["remap"] if isinstance(table, int) else random_table(table[1], k, bits)
            new, bad = index_ref.remap_fast(I, k, tb, bits)
            m.bad = (0 if bad_fresh else m.bad) + bad
            exp.update(cent=cent, index=I, table=tb, out=index_ref.pack_fast(new, bits), bad=m.bad)
    elif name == "optimize":
        i, k, mode, flags, bits = op[1:6]
        assert k >= n_fixed_of(m.fid) and m.n_kept(i, m.wc()) > 0 and bits in (0, 8 * host_format(k, m.t)), op
        if num:
            cent = R.centroids(((i, m.wc()),), k, m.fid, m.w)
            pal, I = R.palette_bytes(cent), R.index(R.img(i), cent, mode, m.t)
            remap, out_pal, info = index_ref.plan(index_ref.usage(I, k), pal, flags)
            b = bits or info[3]
            new, bad = index_ref.remap_fast(I, k, remap, b)
            assert bad == 0
            exp.update(source=pal, index=I, palette=out_pal, info=info, bits=b, out=index_ref.pack_fast(new, b))
    else:
        raise ValueError(op)


def refuse_2(m, op, exp):
    what = op[1]
    if what in ("shared_frame_on_local", "local_tolerance_without_delta", "warm_with_fixed"):
        o = m.seq[op[2]].out
        assert o is not None and o.get("local"), op
        if what == "warm_with_fixed":
            assert o["warm"] and n_fixed_of(m.fid) > 0, op
            exp["status"] = ERR_UNSUPPORTED
            exp["after"], o["failed"] = o["failed"], "fixed_on_warm"
    elif what == "local_frame_on_shared":
        o = m.seq[op[2]].out
        assert o is not None and not o.get("local"), op
    elif what == "local_frame_no_output":
        assert m.seq[op[2]].out is None, op
    elif what in ("local_meld", "local_index8_k256"):
        m.seq[op[2]].out = None                               # a begin ends what was open before it checks its arguments
    elif what in ("plan_indices_above_k", "plan_empty_record"):
        assert m.urec[op[2]] is not None, op
    elif what == "optimize_bits_too_narrow":
        assert op[3] >= max(n_fixed_of(m.fid), 3) and m.n_kept(op[2], m.t) > 0, op
    else:
        assert what == "remap_bad_bits" and op[3] not in BITS, op


def refuse_3(m, op, exp):
    """the refusals of alpha weighting: all KMG_ERR_INVALID_ARGUMENT, none changes anything"""
    what = op[1]
    if what == "weight_bad_value":
        assert op[2] not in (0, 1), op
    elif what == "l_weight_bad_value":
        assert m.lloyd[op[2]] is not None and op[3] not in (0, 1), op
    elif what == "octree_weighted":                           # no other cause applies: the octree under fixed colours is refused too
        assert m.w == 1 and n_fixed_of(m.fid) == 0 and op[4] in (0, 1, 2), op
    elif what == "weighted_no_kept_pixel":                    # alpha mode's error although the cutoff is 0; no k below fixed colours
        assert m.w == 1 and m.t == 0 and n_fixed_of(m.fid) == 0 and op[2] in (0, 1, 2), op
    elif what == "l_weight_under_caller_binding":
        s = m.lloyd[op[2]]
        assert s is not None and s.owner == "caller" and not s.w and op[3] in (0, 1), op
    else:
        # weighted_lftu and weighted_accumulate_into cannot tell two causes apart: a weighted object never holds a binding, so both
        # calls would also be refused as "not bound", with the same status.  They are listed because the header lists them; what
        # they do show is that the refused call writes neither labels nor sums and leaves the object weighted and usable.
        s = m.lloyd[op[2]]
        assert what in ("weighted_bind", "weighted_lftu", "weighted_accumulate_into") and s is not None and s.w and s.k <= 256, op


# ---- surface 4 on the model: a batched call is the per-image call, image by image -------------------------------------
def fmt_bytes(fmt):
    return {None: 4, 0: 4, 1: 1, 2: 2}[fmt]


def batch_resident(shape, t, call, fmt=0):
    """the bytes an image of `shape` keeps on the device while its sub-batch runs, as include/kmeans_hip.h lists them at
    max_resident_bytes: the source (kmg_palette_batch: only where the image is not shrunk), the shrunk copy where it has one, the
    same again under a cutoff for the compacted copy, the output of an indexed call; kmg_find_batch: the source and the output"""
    h, w = shape
    if call == "b_find":
        return (4 + fmt_bytes(fmt)) * w * h
    shrunk = max(w, h) > SHRINK
    sw, sh = O.resized_dims(w, h, SHRINK) if shrunk else (w, h)
    return (4 * sw * sh if shrunk else 0) + (0 if call == "b_palette" and shrunk else 4 * w * h) + (4 * sw * sh if t else 0) + \
        (fmt_bytes(fmt) * w * h if call == "b_reduce_indexed" else 0)


def batch_cut(sizes, bound):
    """the sub-batches of images that keep sizes[i] bytes each: consecutive, filled while the bytes fit `bound` (0 = 1 GiB); an
    image that does not fit alone forms one of its own"""
    bound = bound or 1 << 30
    pieces, held = [], 0
    for i, b in enumerate(sizes):
        if not pieces or held + b > bound:
            pieces.append([])
            held = 0
        pieces[-1].append(i)
        held += b
    return pieces


def batch_output_report(m, n, mode, algo=0):
    """(batched, per_image) of the output step: meld, diffusion, the octree and a forced table strategy keep the per-image pass;
    replace and dither join the launch on this harness's images (the generator leaves the one measured rule out)"""
    per_image = n if mode in (2, 3) or algo == 1 or m.strategy == 2 else 0
    return n - per_image, per_image


def batch_tables(seed, k, n, shared):
    return [gamut_centroids(seed + (0 if shared else j), k)[0] for j in range(1 if shared else n)]


def find_rgba(R, i, pal, mode, t):
    img = R.img(i)
    return R._memo(("find", i, pal.tobytes(), mode, t), lambda: alpha_ref.find(O, img, pal, mode, t) if t else
                   diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(O, pal)) if mode == 3 else O.find(img, pal, mode))


def apply_op_4(m, op, exp):
    name, num, R = op[0], m.numeric, m.ref
    imgs = op[1]
    n = len(imgs)
    shapes = [m.images[i][1].shape[:2] for i in imgs]
    assert n >= 1, op
    if name in BATCH_PALETTE_CALLS:
        k, algo, bound = op[2], op[3], op[-1]
        mode = 0 if name == "b_palette" else op[4]
        fmt = op[5] if name == "b_reduce_indexed" else 0
        assert m.fid == 0 and m.w == 0 and all(m.n_kept(i, m.t) > 0 for i in imgs), op
        assert algo == 0 or (algo == 1 and m.t == 0 and name != "b_reduce_indexed" and mode in (0, 1) and all(max(s) <= SHRINK for s in shapes)), op
        assert (fmt != 1 or k + (1 if m.t else 0) <= 256) and (fmt == 0 or mode != 2), op
        assert not (name == "b_reduce_indexed" and mode == 1 and k >= 128 and any(h * w >= 16384 for h, w in shapes)), op
        pieces = batch_cut([batch_resident(s, m.t, name, fmt) for s in shapes], bound)
        exp["pieces"] = pieces
        if name == "b_reduce_indexed":
            exp["areport"] = batch_output_report(m, n, mode, algo) + (len(pieces),)
        if not num:
            return
        if algo == 1:
            exp["report"] = (0, 0, len(pieces), 0)
            if name == "b_palette":
                exp["palettes"] = [R._memo(("octree", i, k), lambda i=i: O.palette_octree(R.img(i), k)) for i in imgs]
            else:
                exp["outputs"] = [R._memo(("octree", i, k, mode), lambda i=i: O.reduce_octree(R.img(i), k, mode)) for i in imgs]
            return
        steps = [R.palette_step(i, m.t, k) for i in imgs]
        its = [it for _, it in steps]
        # the chain of a sub-batch: k launches of the initialisation, the initial assignment, one launch per iteration up to its
        # slowest image; a sub-batch of one image takes the per-image palette step and launches none
        exp["report"] = (sum(k + 2 + max(its[q] for q in p) for p in pieces if len(p) >= 2), max(its), len(pieces), 0)
        if name == "b_palette":
            exp["palettes"] = [R._memo(("sorted", i, m.t, k), lambda c=c: sorted_palette(c)) for i, (c, _) in zip(imgs, steps)]
        elif name == "b_reduce":
            exp["outputs"] = [R.rgba(R.img(i), c, mode, m.t) for i, (c, _) in zip(imgs, steps)]
        else:
            exp["palettes"] = [R.palette_bytes(c) for c, _ in steps]
            exp["outputs"] = [R.rgba(R.img(i), c, mode, m.t) if fmt == 0 else R.index(R.img(i), c, mode, m.t) for i, (c, _) in zip(imgs, steps)]
    elif name == "b_find":
        k, seed, mode, fmt, bound = op[2:7]
        assert (fmt != 1 or k + (1 if m.t else 0) <= 256) and (fmt == 0 or mode != 2), op
        assert not (mode == 1 and k >= 128 and any(h * w >= 16384 for h, w in shapes)), op
        pieces = batch_cut([batch_resident(s, m.t, name, fmt) for s in shapes], bound)
        exp["pieces"] = pieces
        exp["areport"] = batch_output_report(m, n, mode) + (len(pieces),)
        if num:
            pal = find_palette(seed, k)
            exp["outputs"] = [find_rgba(R, i, pal, mode, m.t) if fmt == 0 else R.index(R.img(i), R.find_centroids(pal), mode, m.t) for i in imgs]
    elif name == "b_palette_device":
        k = op[2]
        assert all(h * w < 1 << 19 for h, w in shapes), op
        if num:
            steps = [R.lloyd_triple(i, k) for i in imgs]
            its = [it for _, it in steps]
            exp.update(cent=[c for c, _ in steps], its=its, report=(k + 2 + max(its), max(its), 1, 0))
    else:
        k, seed, shared, mode, fmt, offs = op[2:8]
        assert name == "b_apply_device" and (fmt != 1 or k + (1 if m.t else 0) <= 256) and (fmt == 0 or mode != 2) and offs in CPAIR_OFFSETS, op
        assert not (mode == 1 and k >= 128 and any(h * w >= 16384 for h, w in shapes)), op
        exp["areport"] = batch_output_report(m, n, mode) + (1,)
        if num:
            tables = batch_tables(seed, k, n, shared)
            exp["tables"] = tables
            exp["outputs"] = [R.rgba(R.img(i), tables[0 if shared else j], mode, m.t) if fmt == 0 else
                              R.index(R.img(i), tables[0 if shared else j], mode, m.t) for j, i in enumerate(imgs)]


def refuse_4(m, op, exp):
    """the refusals of the batched calls: all KMG_ERR_INVALID_ARGUMENT, checked for the whole batch before any output is written"""
    what = op[1]
    if what in ("batch_fixed", "batch_weighted"):
        assert op[2] in BATCH_PALETTE_CALLS and (n_fixed_of(m.fid) > 0 if what == "batch_fixed" else (m.fid == 0 and m.w == 1)), op
    elif what == "batch_no_kept_pixel":
        gone = [j for j, i in enumerate(op[3]) if m.n_kept(i, m.t) == 0]
        assert op[2] in BATCH_PALETTE_CALLS and m.t > 0 and m.fid == 0 and m.w == 0 and gone, op
        exp["needle"] = f"image {gone[0]}:"
    elif what == "batch_index8_full":
        assert op[2] in ("b_find", "b_reduce_indexed", "b_apply_device") and op[4] + (1 if m.t else 0) == 257, op
    elif what == "batch_meld_indexed":
        assert op[2] in ("b_find", "b_reduce_indexed", "b_apply_device") and op[5] in (1, 2), op
    elif what == "batch_bad_tables":
        assert op[4] not in (1, len(op[2])), op
    else:
        assert what == "batch_empty" and op[2] in BATCH_OPS, op


# ---- the runner -----------------------------------------------------------------------------------------------------
def _bits(c):
    return np.ascontiguousarray(c, np.float32).view(np.uint32)


class Runner:
    """executes ops on a backend and compares with the numeric model after every op"""

    def __init__(self, env, seed, seq, counters=None, proc=None, cache=None):
        self.env, self.mem = env, env.mem
        self.images = make_images(seed, seq)
        self.model = Model(self.images, numeric=True, cache=cache)
        self.counters = counters if counters is not None else collections.Counter()
        self.own_proc = proc is None
        self.proc = env.session_processor() if proc is None else proc
        for name, v in (("set_alpha_cutoff", 0), ("set_fixed_colors", None), ("set_strategy", 0), ("set_alpha_weight", False)):
            getattr(self.proc, name)(v)                       # (a caller's processor: a known start)
        self.weighted_closed = False                          # the last Lloyd call closed a weighted object: its block is the idle list's newest
        self.last_quality = None
        self.pix = []
        for _, a in self.images:
            b = self.mem.alloc(a.size)
            self.mem.write(b, 0, a.reshape(-1))
            self.pix.append(b)
        big = 4 << 20
        self.out = self.mem.alloc(big + GUARD)
        self.lab = self.mem.alloc(4 * 60000 + GUARD)
        self.rec = self.mem.alloc(112 + GUARD)
        self.mem.fill(self.rec, 0, 112 + GUARD, PATTERN)
        self.mem.write(self.rec, 0, np.zeros(112, np.uint8))
        self.count = self.mem.alloc(8)
        self.acc, self.obj = [None, None], [None, None]
        self.seqs = [None, None]
        self.pairs = [None, None]
        self.cpairs = [None, None]
        self.urec = [None, None]                              # device usage records: k + 2 uint64 and the guard
        self.out2 = self.mem.alloc((1 << 16) + GUARD)
        self.bad = self.mem.alloc(8 + GUARD)
        self.mem.fill(self.bad, 0, 8 + GUARD, PATTERN)
        self.mem.write(self.bad, 0, np.zeros(8, np.uint8))
        self.coded = [[], []]                                 # what the frames of each Sequence's open output returned
        self.remapped = [{}, {}]
        self.n_ops = 0

    def close(self):
        for o in self.obj + self.seqs:
            if o is not None:
                o.close()
        self.obj, self.seqs = [None, None], [None, None]
        if self.own_proc:
            self.proc.close()

    def fail(self, what, got=None, want=None):
        detail = ""
        if got is not None and want is not None:
            got, want = np.asarray(got), np.asarray(want)
            if got.shape == want.shape:
                bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
                detail = f": {bad.size} of {got.size} differ, first at {bad[:4].tolist()}: got {got.reshape(-1)[bad[:4]].tolist()} want {want.reshape(-1)[bad[:4]].tolist()}"
            else:
                detail = f": shape {got.shape} against {want.shape}"
        raise Mismatch(what + detail)

    def same(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want):
            self.fail(what, got, want)

    def arm(self, buf, nbytes):
        self.mem.fill(buf, 0, nbytes + GUARD, PATTERN)

    def collect(self, buf, nbytes, dtype, what):
        raw = self.mem.read(buf, 0, nbytes + GUARD)
        if not (raw[nbytes:] == PATTERN).all():
            self.fail(f"{what}: written past the end")
        return raw[:nbytes].view(dtype)

    def expect_status(self, status, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except self.env.Error as e:
            if e.status != status:
                self.fail(f"refused with status {e.status}, the header names {status}")
            return
        self.fail(f"a call the header refuses with status {status} was accepted")

    def run(self, ops):
        for i, op in enumerate(ops):
            try:
                self.step(op)
            except Mismatch as e:
                raise Mismatch(f"op {i} {op!r}: {e}") from None
            except self.env.Error as e:
                raise Mismatch(f"op {i} {op!r}: a legal call was refused: {e}") from None
            self.n_ops += 1

    def fixed_arg(self, fid):
        return None if FIXED[fid] is None else np.array(FIXED[fid], np.uint8)

    def count_k(self, k, fmt):
        self.counters[f"k:{k_class(k)}:{ {None: 'rgba8', 0: 'rgba8', 1: 'index8', 2: 'index16'}[fmt] }"] += 1

    def step(self, op):
        env, m, name, C, proc = self.env, self.model, op[0], self.counters, self.proc
        C["op:" + name] += 1
        streams = env.streams
        before_t = m.t
        if name not in ("l_new", "l_re", "l_close"):
            self.weighted_closed = False
        if name.startswith("l_"):
            return self.step_lloyd(op)
        if name.startswith("s_"):
            return self.step_sequence(op)
        if name == "refuse":
            return self.step_refuse(op)
        if m.w and name in ("palette", "reduce", "reduce_indexed", "quality", "optimize"):
            C["weighted_host:" + name] += 1
            C["weighted_host_at_cutoff_0"] += int(m.t == 0)
        if name in ("palette", "reduce", "reduce_indexed", "quality") and op[1] == MAP:
            C["host_call_on_the_map"] += 1
        exp = apply_op(m, op)
        if name == "cutoff":
            proc.set_alpha_cutoff(op[1])
        elif name == "weight":
            proc.set_alpha_weight(bool(op[1]))
        elif name == "motif":
            C["motif:" + op[1]] += 1
        elif name == "fixed":
            C[f"fixed:{op[1]}"] += 1
            proc.set_fixed_colors(self.fixed_arg(op[1]))
        elif name == "strategy":
            proc.set_strategy(op[1])
        elif name == "palette":
            self.count_k(op[2], None)
            self.same("palette", proc.palette(op[2], self.images[op[1]][1], 0), exp["palette"])
        elif name == "reduce":
            self.count_k(op[2], None)
            self.same(f"reduce (mode {op[3]})", proc.reduce(op[2], self.images[op[1]][1], 0, op[3]), exp["image"])
        elif name == "reduce_indexed":
            i, k, mode, cmp = op[1:5]
            pal, idx = proc.reduce_indexed(k, self.images[i][1], 0, mode)
            self.count_k(k, host_format(k, before_t))
            self.same("palette of reduce_indexed", pal, exp["palette"])
            if idx.dtype != index_dtype(host_format(k, before_t)):
                self.fail(f"index type {idx.dtype}")
            self.same(f"index map of reduce_indexed (mode {mode})", idx.astype(np.int64), exp["index"])
            if cmp:                                       # the just-produced output against its source: both forms give one record
                C["compare_host"] += 1
                src = self.images[i][1]
                want = m.ref.stats(src, exp["index"], exp["palette"], before_t, 3)
                self.same("compare of an index map", proc.compare(src, idx, palette=pal).as_tuple(), want)
                self.same("compare of the image", proc.compare(src, exp["image"]).as_tuple(), want)   # (index k: on uncounted pixels only)
        elif name == "find":
            self.same(f"find (mode {op[3]})", proc.find(self.images[op[1]][1], find_palette(op[4], op[2]), op[3]), exp["image"])
        elif name == "find_indexed":
            self.count_k(op[2], host_format(op[2], before_t))
            got = proc.find_indexed(self.images[op[1]][1], find_palette(op[4], op[2]), op[3])
            self.same(f"find_indexed (mode {op[3]})", got.astype(np.int64), exp["index"])
        elif name == "quality":
            i, dE, k_min, k_max, mode, indexed = op[1:7]
            k, pal, out, stats, reached = proc.reduce_quality(self.images[i][1], dE, k_min, k_max, mode, bool(indexed))
            if (k, reached) != (exp["k"], exp["reached"]):
                self.fail(f"reduce_quality chose k = {k}, reached = {reached}; the model k = {exp['k']}, reached = {exp['reached']}")
            self.same("palette of reduce_quality", pal, exp["palette"])
            self.same("record of reduce_quality", stats.as_tuple(), exp["stats"])
            self.same("output of reduce_quality", out.astype(np.int64) if indexed else out, exp["out"])
            if self.last_quality is not None and self.last_quality[0] == op[1:] and self.last_quality[1] != m.w:
                C["quality_weighting_changes_the_palette"] += int(not np.array_equal(self.last_quality[2], exp["palette"]))
            self.last_quality = (op[1:], m.w, exp["palette"])
            if op[7]:                                     # the switches are as they were: the same call again gives the same answer
                k2, pal2, out2, _, _ = proc.reduce_quality(self.images[i][1], dE, k_min, k_max, mode, bool(indexed))
                self.same("reduce_quality, again", out2.astype(np.int64) if indexed else out2, exp["out"])
        elif name in ("apply", "apply_plan"):
            self.step_apply(op, exp, before_t)
        elif name == "compact":
            i, cut, s = op[1:4]
            n = self.images[i][1].shape[0] * self.images[i][1].shape[1]
            self.arm(self.out, 4 * n)
            proc.alpha_compact(self.pix[i].ptr, n, cut, self.out.ptr, self.count.ptr, streams[s])
            env.sync()
            got_n = int(self.mem.read(self.count, 0, 8).view(np.uint64)[0])
            if got_n != exp["kept"].shape[0]:
                self.fail(f"alpha_compact kept {got_n}, the model {exp['kept'].shape[0]}")
            raw = self.collect(self.out, 4 * n, np.uint8, "alpha_compact")
            self.same("alpha_compact", raw[:4 * got_n].reshape(-1, 4), exp["kept"])
            if not (raw[4 * got_n:] == PATTERN).all():
                self.fail("alpha_compact wrote behind the kept pixels")
        elif name == "compare_device":
            self.step_compare(op, exp, before_t)
        elif name == "pair_open":
            P, fam, fmt, k = op[1:5]
            self.count_k(k, fmt)
            pr = m.pairs[P]
            h, w = pr["canvas"].shape
            n, size = w * h, fmt
            C["pair_reopened"] += int(self.pairs[P] is not None)
            bufs = {"index": self.mem.alloc(size * n + GUARD), "canvas": self.mem.alloc(size * n + GUARD), "delta": self.mem.alloc(size * n + GUARD),
                    "held": self.mem.alloc(4 * n + GUARD), "rec": self.mem.alloc(48 + GUARD)}
            for b, nb in (("canvas", size * n), ("held", 4 * n), ("rec", 48)):
                self.arm(bufs[b], nb)
            self.mem.write(bufs["canvas"], 0, np.full(n, k, index_dtype(fmt)))
            self.mem.write(bufs["held"], 0, np.zeros(4 * n, np.uint8))
            self.pairs[P] = bufs
        elif name == "pair_frame":
            self.step_pair_frame(op, exp, before_t)
        elif name in ("cpair_open", "cpair_frame"):
            self.step_cpair(op, exp)
        elif name in ("usage_device", "plan", "remap_device", "optimize"):
            self.step_index(op, exp, before_t)
        elif name in BATCH_OPS:
            self.step_batch(op, exp)
        else:
            raise ValueError(op)

    # -- output passes under the switches
    def check_output(self, what, fmt, w, h, exp_out):
        size = {None: 4, 1: 1, 2: 2}[fmt]
        if fmt is None:
            self.same(what, self.collect(self.out, 4 * w * h, np.uint8, what).reshape(h, w, 4), exp_out)
        else:
            self.same(what, self.collect(self.out, size * w * h, index_dtype(fmt), what).astype(np.int64).reshape(h, w), exp_out)

    def step_apply(self, op, exp, t0):
        env, proc, C = self.env, self.proc, self.counters
        i, mode, fmt, k, seed = op[1:6]
        s = op[-1]
        self.count_k(k, fmt)
        img = self.images[i][1]
        h, w = img.shape[:2]
        size = {None: 4, 1: 1, 2: 2}[fmt]
        self.arm(self.out, size * w * h)
        p = self.pix[i].ptr
        if op[0] == "apply_plan":
            C["plan_outlives_cutoff"] += 1
            pl = proc.apply_plan(exp["cent"], mode, w * h, env.streams[s], format=fmt)
            try:
                proc.set_alpha_cutoff(op[6])              # the plan keeps the cutoff it was made under
                r = 1 + seed % (h - 1) if h > 1 else 1
                pl.run(p, w, r, 0, self.out.ptr, env.streams[s])
                if h > r:
                    pl.run(p + 4 * r * w, w, h - r, r, self.out.ptr + size * r * w, env.streams[1 - s])
                env.sync()
                pl.status()
            finally:
                pl.close()
        else:
            proc.apply(p, w, h, 0, exp["cent"], mode, self.out.ptr, env.streams[s], format=fmt)
        env.sync()
        self.check_output(f"{op[0]} (mode {mode}, format {fmt}, cutoff {t0})", fmt, w, h, exp["out"])

    def step_compare(self, op, exp, t0):
        env, proc, C = self.env, self.proc, self.counters
        i, other, fmt, k, seed, nb, order, cut, what, fresh, s = op[1:12]
        self.count_k(k, fmt)
        img = self.images[i][1]
        h, w = img.shape[:2]
        size = {None: 4, 1: 1, 2: 2}[fmt]
        self.arm(self.out, size * w * h)
        proc.apply(self.pix[i].ptr, w, h, 0, exp["cent"], 0, self.out.ptr, env.streams[s], format=fmt)
        env.sync()
        self.check_output("the output compare_device measures", fmt, w, h, exp["out"])
        if fresh:
            self.mem.write(self.rec, 0, np.zeros(112, np.uint8))
        else:
            C["record_combined_across_images"] += 1
        bands = bands_of(h, nb, order)
        C[f"compare_bands:{len(bands)}"] += 1
        for j, (r0, rows) in enumerate(bands):
            proc.compare_device(self.pix[i].ptr + 4 * r0 * w, self.out.ptr + size * r0 * w, rows * w, self.rec.ptr, format=0 if fmt is None else fmt,
                                palette=exp["palette"], alpha_cutoff=cut, what=what, stream=env.streams[(s + j) % 2])
        env.sync()
        got = tuple(int(v) for v in self.collect(self.rec, 112, np.uint64, "error record"))
        self.same("error record", got, exp["record"])

    def step_pair_frame(self, op, exp, t0):
        env, proc, C, m = self.env, self.proc, self.counters, self.model
        P, i, tol, nb, order, s = op[1:7]
        pr, bufs = m.pairs[P], self.pairs[P]
        fmt, k = pr["fmt"], pr["k"]
        img = self.images[i][1]
        h, w = img.shape[:2]
        n, size, dt = w * h, fmt, index_dtype(fmt)
        C["pair_exact" if tol is None else "pair_lossy"] += 1
        self.arm(bufs["index"], size * n)
        self.arm(bufs["delta"], size * n)
        proc.apply(self.pix[i].ptr, w, h, 0, exp["cent"], pr["mode"], bufs["index"].ptr, env.streams[s], format=fmt)
        env.sync()
        self.same("index map of the frame", self.collect(bufs["index"], size * n, dt, "index map").astype(np.int64).reshape(h, w), exp["index"])
        fresh = np.array(hold_ref.FRESH[:2], np.uint64).tobytes() + np.array(hold_ref.FRESH[2:6], np.uint32).tobytes() + \
            np.array(hold_ref.FRESH[6:], np.uint64).tobytes()
        self.mem.write(bufs["rec"], 0, np.frombuffer(fresh, np.uint8).copy())
        bands = bands_of(h, nb, order)
        C[f"delta_bands:{len(bands)}"] += 1
        for j, (r0, rows) in enumerate(bands):
            a, e = 4 * r0 * w, size * r0 * w
            stj = env.streams[(s + j) % 2]
            if tol is None:
                proc.frame_delta(bufs["index"].ptr + e, bufs["canvas"].ptr + e, w, rows, r0, fmt, k, bufs["delta"].ptr + e, bufs["rec"].ptr, stj)
            else:
                proc.frame_delta_lossy(self.pix[i].ptr + a, bufs["index"].ptr + e, bufs["canvas"].ptr + e, bufs["held"].ptr + a, w, rows, r0, fmt, k, tol,
                                       bufs["delta"].ptr + e, bufs["rec"].ptr, stj)
        env.sync()
        if tol is None:
            self.mem.write(bufs["held"], 0, img.reshape(-1))             # the canvas equals the map: the held source is this frame
        raw = self.collect(bufs["rec"], 48, np.uint8, "frame record")
        got = tuple(int(v) for v in raw[:16].view(np.uint64)) + tuple(int(v) for v in raw[16:32].view(np.uint32)) + \
            tuple(int(v) for v in raw[32:48].view(np.uint64))
        self.same("frame record", got, exp["record"])
        self.same("delta map", self.collect(bufs["delta"], size * n, dt, "delta map").astype(np.int64).reshape(h, w), exp["delta"])
        self.same("canvas", self.collect(bufs["canvas"], size * n, dt, "canvas").astype(np.int64).reshape(h, w), exp["canvas"])
        self.same("held source", self.collect(bufs["held"], 4 * n, np.uint8, "held source").reshape(h, w, 4), exp["held"])

    # -- Lloyd objects
    def step_lloyd(self, op):
        env, m, name, C = self.env, self.model, op[0], self.counters
        L = op[1]
        o = self.obj[L]
        if name in ("l_new", "l_re"):
            if name == "l_re":
                o.close()
            C[f"lloyd_k:{k_class(op[2])}"] += 1
            if name == "l_re":
                self.weighted_closed = bool(m.lloyd[L].w)
            C["lloyd_object_created_right_after_a_weighted_one_closed"] += int(self.weighted_closed)    # (no call between the two)
            self.weighted_closed = False
            apply_op(m, op)
            self.obj[L] = env.lloyd(self.proc, op[2])
            self.acc[L] = self.mem.alloc(32 * op[2] + GUARD)
            self.mem.fill(self.acc[L], 32 * op[2], GUARD, PATTERN)
            self.mem.write(self.acc[L], 0, np.zeros(32 * op[2], np.uint8))
            return
        if name == "l_close":
            self.weighted_closed = bool(m.lloyd[L].w)
            apply_op(m, op)
            o.close()
            self.obj[L] = None
            return
        s = m.lloyd[L]
        st = env.streams[op[-1]] if name not in ("l_set", "l_fix") else env.streams[0]
        acc = self.acc[L].ptr
        img_i = op[2] if name in LLOYD_IMAGE_OPS else None
        if img_i is not None:
            h, w = self.images[img_i][1].shape[:2]
            n, p = w * h, self.pix[img_i].ptr
        f_before = s.f
        exp = apply_op(m, op)
        if exp.get("unbind"):
            o.unbind_image()                                  # (whether a pass on other pixels re-binds is the cost model's)
        if name in ("l_assign", "l_assign_update", "l_iterate", "l_run"):
            C[f"pass:{name}:{'weighted' if s.w else 'unweighted'}"] += 1
            C["lloyd_pass_on_the_map"] += int(img_i == MAP)
        if f_before and name in ("l_update", "l_assign_update", "l_iterate", "l_run", "l_lftu"):
            C["update_with_n_fixed:" + name] += 1
        if name == "l_set":
            o.set_centroids(s.cent, st)
        elif name == "l_init":
            C[f"seeds:{op[3]}"] += 1
            o.init_centroids_seeded(p, w, h, fixed_ref.pins_lab(O, np.array(FIXED[3], np.uint8)[:op[3]]), st)
        elif name == "l_fix":
            C["set_fixed_zero" if op[2] == 0 else "set_fixed"] += 1
            o.set_fixed(op[2])
        elif name == "l_bind":
            o.bind_image(p, n, st)
        elif name == "l_unbind":
            o.unbind_image()
        elif name == "l_weight":
            C[f"l_weight:{op[2]}:owner_{exp['owner'] or 'nobody'}"] += 1
            o.set_weighting(op[2])
        elif name == "l_conv":
            got = o.converged_count(st)
            if got != exp["nconv"]:
                self.fail(f"converged_count {got}, expected {exp['nconv']}")
        elif name == "l_update":
            o.update(acc, st)
        elif name == "l_assign":
            self.arm(self.lab, 4 * n)
            o.assign_accumulate(p, n, self.lab.ptr, acc, st)
        elif name == "l_assign_update":
            self.arm(self.lab, 4 * n)
            o.assign_update(p, n, self.lab.ptr if op[3] else 0, acc, bool(op[4]), st)
        elif name == "l_iterate":
            self.arm(self.lab, 4 * n)
            for _ in range(op[3]):
                o.iterate(p, n, self.lab.ptr, acc, True, st)
            o.flush(st)
        elif name == "l_run":
            self.arm(self.lab, 4 * n)
            it = o.run(p, n, self.lab.ptr if op[3] else 0, st)
            if it != exp["iterations"]:
                self.fail(f"run stopped at iteration {it}, the model at {exp['iterations']}")
        elif name == "l_lftu":
            self.arm(self.lab, 4 * n)
            self.mem.write(self.acc[L], 0, np.zeros(32 * s.k, np.uint8))
            o.bind_image(p, n, st)
            o.accumulate_into(p, n, acc, st)
            o.labels_from_tables_update(p, n, self.lab.ptr, acc, st)
        env.sync()
        if "labels" in exp:
            self.same("labels of " + name, self.collect(self.lab, 4 * n, np.uint32, "labels"), exp["labels"])
        got = self.collect(self.acc[L], 32 * s.k, np.int64, "accumulators").reshape(s.k, 4)
        self.same("accumulators", got, s.acc)
        if s.w and name in ("l_assign", "l_assign_update", "l_iterate"):
            pixels = m.ref.assign(img_i, exp["cent_before"], 0)[1][:, 3] if "cent_before" in exp else None
            if pixels is not None:
                C["free_cluster_of_weight_0_with_pixels"] += int(((s.acc[s.f:, 3] == 0) & (pixels[s.f:] > 0)).any())
                C["pinned_cluster_of_weight_0_with_pixels"] += int(((s.acc[:s.f, 3] == 0) & (pixels[:s.f] > 0)).any())
        if exp.get("cent") is not None:
            got = o.get_centroids(st)
            if not np.array_equal(_bits(got), _bits(exp["cent"])):
                self.fail("centroid bits", _bits(got), _bits(exp["cent"]))

    # -- Sequence objects
    def step_sequence(self, op):
        env, m, name, C = self.env, self.model, op[0], self.counters
        S = op[1]
        q = self.seqs[S]
        if name in ("s_new", "s_close", "s_output", "s_output_local", "s_end"):
            self.coded[S], self.remapped[S] = [], {}
        if name == "s_new":
            apply_op(m, op)
            self.seqs[S] = self.proc.sequence()
            return
        if name == "s_close":
            C["closed_with_output_open"] += int(m.seq[S].out is not None)
            apply_op(m, op)
            q.close()
            self.seqs[S] = None
            return
        if name in ("s_centroids", "s_palette", "s_output"):
            C["sequence_loop_weighted" if m.w else "sequence_loop_unweighted"] += 1
            C["sequence_loop_weighting_differs_from_an_add"] += int(any(w != m.w for w in m.seq[S].wadd))
        if name == "s_output":
            C["reoutput"] += int(m.seq[S].out is not None)
            C["mixed_cutoff_sequence"] += int(len({t for _, t in m.seq[S].frames}) > 1)
            self.count_k(op[2], op[4])
        exp = apply_op(m, op)
        if name == "s_add":
            i = op[2]
            h, w = self.images[i][1].shape[:2]
            C["add_shrunk"] += int(max(w, h) > SHRINK)
            C["add_under_weighting"] += int(m.w)
            C["add_under_weighting_loses_weight_0_pixels"] += int(m.w and m.t == 0 and m.n_kept(i, 1) < w * h)
            if op[3]:
                q.add_device(self.pix[i].ptr, w, h, env.streams[op[4]])
            else:
                q.add(self.images[i][1])
        elif name == "s_clear":
            q.clear()
        elif name == "s_info":
            if tuple(q.info()) != exp["info"]:
                self.fail(f"info {tuple(q.info())}, the model {exp['info']}")
        elif name == "s_centroids":
            C["mixed_cutoff_sequence"] += int(len({t for _, t in m.seq[S].frames}) > 1)
            got = q.centroids(op[2])
            if not np.array_equal(_bits(got), _bits(exp["cent"])):
                self.fail("centroid bits of the sequence", _bits(got), _bits(exp["cent"]))
        elif name == "s_palette":
            C["mixed_cutoff_sequence"] += int(len({t for _, t in m.seq[S].frames}) > 1)
            self.same("palette of the sequence", q.palette(op[2]), exp["palette"])
        elif name == "s_output":
            o = m.seq[S].out
            h, w = o["shape"]
            self.same("palette of the output", q.output(o["k"], o["mode"], o["fmt"], w, h), exp["palette"])
        elif name == "s_end":
            q.end_output()
        elif name == "s_frame":
            i, delta, tol = op[2:5]
            C["frame_exact" if tol is None else "frame_lossy"] += 1
            if exp["transition"]:
                C["transition:" + exp["transition"]] += 1
            got, info, full = q.frame(self.images[i][1], delta=bool(delta), tolerance=tol)
            C["is_full_fallback"] += int(exp.get("fallback", False))
            C["frame_held_pixels"] += int(tol is not None and exp["record"][6] > 0)
            if bool(full) != exp["full"]:
                self.fail(f"is_full {full}, the model {exp['full']}")
            self.same("frame record", info.as_tuple(), exp["record"])
            self.same("frame map", got if got.ndim == 3 else got.astype(np.int64), exp["map"])
            if got.ndim == 2:
                self.coded[S].append((got, None, bool(full)))
        elif name == "s_output_local":
            k, mode, fmt, fam, warm = op[2:7]
            self.count_k(k, fmt)
            C["local_begin_warm" if warm else "local_begin_cold"] += 1
            h, w = m.seq[S].out["shape"]
            q.output_local(k, mode, fmt, w, h, warm=bool(warm))
        elif name == "s_frame_local":
            self.step_frame_local(op, exp)
        elif name == "s_usage":
            rec, fresh, j = op[2:5]
            k = m.seq[S].out["k"]
            C["s_usage_fresh" if fresh else "s_usage_combined"] += 1
            self.same("usage record (host)", self.host_usage(rec, fresh, k, lambda use: self.proc.index_usage(self.coded[S][j][0], k, use)), exp["counts"])
        elif name == "s_remap":
            slot, bits, j, sure = op[2:6]
            k, tb = m.seq[S].out["k"], m.tables[slot]
            C[f"remap_bits:{bits}"] += 1
            out, bad = self.proc.index_remap(self.coded[S][j][0], k, tb["remap"], bits)
            self.same("remapped map (host)", out, exp["out"])
            if bad != exp["bad"] or (sure and bad):
                self.fail(f"index_remap counted {bad} bad pixels, the model {exp['bad']}" +
                          (", the plan of these maps' own counts drops no used entry" if sure else ""))
            self.remapped[S][j] = (exp["new"], slot)
            coded = self.coded[S]
            if sure and m.seq[S].out.get("cent") is not None and all(self.remapped[S].get(x, (None, None))[1] == slot for x in range(len(coded))):
                # the remapped maps through the pruned palette show what the originals show through the original one
                C["optimize_path_replayed"] += 1
                pal = m.ref.palette_bytes(m.seq[S].out["cent"])
                n_colors, _, transparent, _ = tb["info"]
                if transparent != n_colors:
                    self.fail("the passage plans without TRANSPARENT_FIRST")
                a = local_ref.replay_colour([(mp, pal, full) for mp, _, full in coded], k)
                b = local_ref.replay_colour([(self.remapped[S][x][0], tb["palette"][:n_colors], coded[x][2]) for x in range(len(coded))], n_colors)
                for x in range(len(coded)):
                    self.same(f"canvas after frame {x}, remapped against original", b[x], a[x])
        else:
            raise ValueError(op)

    def host_usage(self, rec, fresh, k, call):
        """a host call that COMBINES into the caller's record `rec`, which lives on the device between the calls"""
        if fresh:
            self.new_record(rec, k)
        use = self.mem.read(self.urec[rec], 0, 8 * (k + 2)).view(np.uint64).copy()
        call(use)
        self.mem.write(self.urec[rec], 0, use)
        return self.read_record(rec, k)

    def new_record(self, rec, k):
        self.urec[rec] = self.mem.alloc(8 * (k + 2) + GUARD)
        self.mem.fill(self.urec[rec], 0, 8 * (k + 2) + GUARD, PATTERN)
        self.mem.write(self.urec[rec], 0, np.zeros(k + 2, np.uint64))

    def read_record(self, rec, k):
        return self.collect(self.urec[rec], 8 * (k + 2), np.uint64, "usage record")

    def step_frame_local(self, op, exp):
        m, C = self.model, self.counters
        S, i, delta, tol = op[1:5]
        q, o = self.seqs[S], m.seq[S].out
        img = self.images[i][1]
        if exp["failed"]:
            C["failed_frame:" + exp["failed"]] += 1
            self.expect_status(exp["status"], q.frame_local, img, delta=bool(delta), tolerance=tol)
            return
        if exp["after"]:
            C["frame_after_failed:" + exp["after"]] += 1
        C["local_warm" if exp["warm"] else "local_cold"] += 1
        C["local_exact" if tol is None else "local_lossy"] += 1
        C["local_first_frame_lossy"] += int(exp["first_lossy"])
        C["local_lossy_full"] += int(exp.get("lossy_full", False))
        C["local_held_pixels"] += int(exp["held_pixels"])
        C["local_cutoff_differs_from_last_frame"] += int(o.get("t_last") not in (None, m.t))
        o["t_last"] = m.t
        if m.w:
            C["local_warm_weighted" if exp["warm"] else "local_cold_weighted"] += 1
        C["local_warm_weighting_differs_from_last_frame"] += int(exp["warm"] and o.get("w_last") not in (None, m.w))
        o["w_last"] = m.w
        got, pal, info, full = q.frame_local(img, delta=bool(delta), tolerance=tol)
        what = f"local frame ({'warm' if exp['warm'] else 'cold'}, cutoff {m.t})"
        self.same("palette of the " + what, pal, exp["palette"])
        if bool(full) != exp["full"]:
            self.fail(f"is_full {full}, the model {exp['full']}")
        self.same("record of the " + what, info.as_tuple(), exp["record"])
        self.same("map of the " + what, got.astype(np.int64), exp["map"])
        self.coded[S].append((got, pal, bool(full)))
        self.same("replay of the coded frames since the begin", local_ref.replay_colour(self.coded[S], o["k"])[-1], exp["shown"])

    def step_refuse(self, op):
        m, proc = self.model, self.proc
        exp = apply_op(m, op)
        what = op[1]
        self.counters["refusal:" + what] += 1
        st = exp["status"]
        if what in REFUSALS_2:
            return self.step_refuse_2(op, st)
        if what in REFUSALS_3:
            return self.step_refuse_3(op, st)
        if what in REFUSALS_4:
            return self.step_refuse_4(op, exp)
        if what == "k_below_fixed_palette":
            self.expect_status(st, proc.palette, op[3], self.images[op[2]][1], 0)
        elif what == "k_below_fixed_reduce":
            self.expect_status(st, proc.reduce, op[3], self.images[op[2]][1], 0, 0)
        elif what == "octree_fixed":
            self.expect_status(st, proc.palette, op[3], self.images[op[2]][1], 1)
        elif what in ("k_below_fixed_sequence", "empty_sequence"):
            self.expect_status(st, self.seqs[op[2]].palette, op[3])
        elif what == "frame_no_output":
            self.expect_status(st, self.seqs[op[2]].frame, self.images[op[3]][1], delta=True)
        elif what == "delta_on_rgba8":
            self.expect_status(st, self.seqs[op[2]].frame, self.images[op[3]][1], delta=True)
        elif what == "lossy_on_rgba8":
            self.expect_status(st, self.seqs[op[2]].frame, self.images[op[3]][1], delta=True, tolerance=40)
        elif what == "lossy_without_delta":
            self.expect_status(st, self.seqs[op[2]].frame, self.images[op[3]][1], delta=False, tolerance=40)
        elif what in ("index8_full", "meld_indexed"):
            i = op[2]
            h, w = self.images[i][1].shape[:2]
            cent, _ = gamut_centroids(7, op[3])
            self.arm(self.out, 2 * w * h)
            self.expect_status(st, proc.apply, self.pix[i].ptr, w, h, 0, cent, 2 if what == "meld_indexed" else 0, self.out.ptr, self.env.streams[0],
                               format=1 if what == "index8_full" else 2)
            self.env.sync()
            if not (self.collect(self.out, 2 * w * h, np.uint8, "refused call") == PATTERN).all():
                self.fail("a refused call wrote output")
        else:
            raise ValueError(op)


    # -- surface 3
    def step_refuse_3(self, op, st):
        m, proc, env, what = self.model, self.proc, self.env, op[1]
        if what == "weight_bad_value":
            self.expect_status(st, env.set_weighting, proc, op[2])
        elif what in ("octree_weighted", "weighted_no_kept_pixel"):
            img, k, algo, variant = (self.images[op[2]][1], op[3], 1, op[4]) if what == "octree_weighted" else (self.images[CLEAR][1], 4, 0, op[2])
            self.counters[f"{what}:{('palette', 'reduce', 'reduce_indexed')[variant]}"] += 1
            if variant == 0:
                self.expect_status(st, proc.palette, k, img, algo)
            elif variant == 1:
                out = np.full(img.shape, PATTERN, np.uint8)
                self.expect_status(st, proc.reduce, k, img, algo, 0, out=out)
                if not (out == PATTERN).all():
                    self.fail("a refused call wrote output")
            else:
                self.expect_status(st, proc.reduce_indexed, k, img, algo, 0)
        else:
            L = op[2]
            o, s = self.obj[L], m.lloyd[L]
            if what in ("l_weight_bad_value", "l_weight_under_caller_binding"):
                if what == "l_weight_under_caller_binding":
                    self.counters[f"l_weight:{op[3]}:owner_caller"] += 1
                self.expect_status(st, o.set_weighting, op[3])
            else:
                h, w = self.images[op[3]][1].shape[:2]
                n, p, stream = w * h, self.pix[op[3]].ptr, env.streams[0]
                self.arm(self.lab, 4 * n)
                if what == "weighted_bind":
                    self.expect_status(st, o.bind_image, p, n, stream)
                elif what == "weighted_accumulate_into":
                    self.expect_status(st, o.accumulate_into, p, n, self.acc[L].ptr, stream)
                else:
                    self.expect_status(st, o.labels_from_tables_update, p, n, self.lab.ptr, self.acc[L].ptr, stream)
                env.sync()
                if not (self.collect(self.lab, 4 * n, np.uint8, "refused call") == PATTERN).all():
                    self.fail("a refused call wrote labels")
            self.same("accumulators after a refused call", self.collect(self.acc[L], 32 * s.k, np.int64, "accumulators").reshape(s.k, 4), s.acc)

    # -- surface 4: the batched calls
    ARMED32 = 0xA5A5A5A5

    def batch_args(self, call, imgs, k, algo=0, mode=0, fmt=0, bound=0, seed=7, shared=1, offs=0, n_images=None, n_tables=None):
        """the arguments of one batched call, every output armed: host outputs are arrays with guard bytes behind them, device
        outputs lie `offs` elements into sentinel-filled allocations, counts and reports hold a pattern"""
        n = len(imgs)
        shapes = [self.images[i][1].shape[:2] for i in imgs]
        size = fmt_bytes(fmt)
        a = dict(call=call, n=n if n_images is None else n_images, k=k, algo=algo, mode=mode, fmt=fmt, bound=bound, stream=self.env.streams[0],
                 ws=[w for _, w in shapes], hs=[h for h, _ in shapes], rep=np.full(4, self.ARMED32, np.uint32),
                 arep=np.full(4, self.ARMED32, np.uint32), offs=offs * size)
        if call in ("b_palette_device", "b_apply_device"):
            a["src"] = [self.pix[i].ptr for i in imgs]
        else:
            a["src"] = [self.images[i][1].ctypes.data for i in imgs]
            a["room"] = [4 * k if call == "b_palette" else size * w * h for h, w in shapes]
            a["out_bufs"] = [np.full(nb + GUARD, PATTERN, np.uint8) for nb in a["room"]]
            a["out"] = [b.ctypes.data for b in a["out_bufs"]]
        if call in ("b_palette", "b_reduce_indexed"):
            a["counts"] = np.full(n, self.ARMED32, np.uint32)
        if call == "b_reduce_indexed":
            a["pal_bufs"] = [np.full(4 * k + GUARD, PATTERN, np.uint8) for _ in imgs]
            a["pal_out"] = [b.ctypes.data for b in a["pal_bufs"]]
        if call == "b_find":
            a["palette"] = np.ascontiguousarray(find_palette(seed, k), np.uint8)
        if call == "b_palette_device":
            a["cent"], a["its"] = np.full((n, k, 4), -7.25, np.float32), np.full(n, self.ARMED32, np.uint32)
        if call == "b_apply_device":
            a["c4"] = np.ascontiguousarray(np.stack(batch_tables(seed, k, n, shared)), np.float32)
            a["n_tables"] = a["c4"].shape[0] if n_tables is None else n_tables
            a["room"] = [size * w * h for h, w in shapes]
            a["dev_bufs"] = [self.mem.alloc(a["offs"] + nb + GUARD) for nb in a["room"]]
            for b, nb in zip(a["dev_bufs"], a["room"]):
                self.mem.fill(b, 0, a["offs"] + nb + GUARD, PATTERN)
            a["out"] = [b.ptr + a["offs"] for b in a["dev_bufs"]]
        return a

    def batch_bodies(self, a):
        """the bodies of the outputs of a batched call, after the bytes around them were seen to be untouched"""
        bodies = []
        for j, nb in enumerate(a["room"]):
            if "dev_bufs" in a:
                raw = self.mem.read(a["dev_bufs"][j], 0, a["offs"] + nb + GUARD)
            else:
                raw = a["out_bufs"][j]
            off = a["offs"] if "dev_bufs" in a else 0
            if not ((raw[:off] == PATTERN).all() and (raw[off + nb:] == PATTERN).all()):
                self.fail(f"output {j} of the batch: written outside the buffer")
            bodies.append(raw[off:off + nb])
        return bodies

    def batch_untouched(self, a):
        """after a refusal: no output, count, palette, centroid or report was written"""
        if "room" in a and not all((b == PATTERN).all() for b in self.batch_bodies(a)):
            self.fail("a refused batch wrote output")
        for name in ("counts", "its", "rep", "arep"):
            if name in a and not (a[name] == self.ARMED32).all():
                self.fail(f"a refused batch wrote {name}")
        if "pal_bufs" in a and not all((b == PATTERN).all() for b in a["pal_bufs"]):
            self.fail("a refused batch wrote a palette")
        if "cent" in a and not (a["cent"] == -7.25).all():
            self.fail("a refused batch wrote centroids")

    def sources_intact(self, imgs):
        """the resident images a device batch read: the neighbouring device buffers of its state and outputs"""
        for i in set(imgs):
            a = self.images[i][1]
            if not np.array_equal(self.mem.read(self.pix[i], 0, a.size), a.reshape(-1)):
                self.fail(f"the resident image {i} changed under a device batch")

    def typed(self, body, shape, fmt):
        h, w = shape
        return body.reshape(h, w, 4) if fmt == 0 else body.view(index_dtype(fmt)).astype(np.int64).reshape(h, w)

    def step_batch(self, op, exp):
        env, C, m, call = self.env, self.counters, self.model, op[0]
        imgs = op[1]
        n = len(imgs)
        shapes = [self.images[i][1].shape[:2] for i in imgs]
        C[f"batch_len:{n if n < 3 else '3+'}"] += 1
        C["batch_repeated_image"] += int(len(set(imgs)) < n)
        C["batch_under_cutoff"] += int(m.t > 0)
        C["batch_under_forced_table"] += int(m.strategy == 2)
        if call in BATCH_PALETTE_CALLS or call == "b_find":
            bound = op[-1]
            C[f"bound:{'0' if bound == 0 else '1' if bound == 1 else 'pairs'}"] += 1
            C["bound_cuts"] += int(len(exp["pieces"]) > 1)
            C["bound_pairs_cuts_twice"] += int(bound > 1 and len(exp["pieces"]) >= 3)
        if call in BATCH_PALETTE_CALLS:
            C["batch_octree" if op[3] else "batch_kmeans"] += 1
            C[f"batch_k:{k_class(op[2])}"] += 1
        if call == "b_palette":
            a = self.batch_args(call, imgs, op[2], algo=op[3], bound=op[4])
        elif call == "b_reduce":
            a = self.batch_args(call, imgs, op[2], algo=op[3], mode=op[4], bound=op[5])
        elif call == "b_reduce_indexed":
            a = self.batch_args(call, imgs, op[2], algo=op[3], mode=op[4], fmt=op[5], bound=op[6])
        elif call == "b_find":
            a = self.batch_args(call, imgs, op[2], seed=op[3], mode=op[4], fmt=op[5], bound=op[6])
        elif call == "b_palette_device":
            a = self.batch_args(call, imgs, op[2])
        else:
            a = self.batch_args(call, imgs, op[2], seed=op[3], shared=op[4], mode=op[5], fmt=op[6], offs=op[7])
            C["tables:shared" if op[4] else "tables:per_image"] += 1
            C[f"batch_offset:{op[7]}"] += 1
        if call in ("b_reduce_indexed", "b_find", "b_apply_device"):
            C[f"batch_output:{('rgba8', 'index8', 'index16')[a['fmt']]}:{('replace', 'dither', 'meld', 'diffuse')[a['mode']]}"] += 1
        status, message = env.batch(self.proc, a)
        env.sync()
        if status != 0:
            self.fail(f"a legal batched call was refused with status {status}: {message}")
        if "report" in exp:
            if tuple(int(v) for v in a["rep"]) != exp["report"]:
                self.fail(f"batch report {tuple(int(v) for v in a['rep'])}, the model {exp['report']} (launches, iterations, sub_batches, fallback)")
            C["batch_iterations_differ"] += int("its" in exp and len(set(exp["its"])) > 1)
        if "areport" in exp:
            launches, batched, per_image, subs = (int(v) for v in a["arep"])
            if (batched, per_image, subs) != exp["areport"] or (launches > 0) != (batched > 0):
                self.fail(f"output report {(launches, batched, per_image, subs)}, the model (launches, batched, per_image, sub_batches) = "
                          f"({'> 0' if exp['areport'][0] else 0}, {exp['areport'][0]}, {exp['areport'][1]}, {exp['areport'][2]})")
        if call == "b_palette_device":
            self.same("iteration counts of the device batch", a["its"].astype(np.int64), np.array(exp["its"], np.int64))
            for j in range(n):
                if not np.array_equal(_bits(a["cent"][j]), _bits(exp["cent"][j])):
                    self.fail(f"centroid bits of image {j} of the device batch", _bits(a["cent"][j]), _bits(exp["cent"][j]))
            return self.sources_intact(imgs)
        bodies = self.batch_bodies(a)
        if call == "b_palette":
            self.same("out_counts of the batch", a["counts"].astype(np.int64), np.array([p.shape[0] for p in exp["palettes"]], np.int64))
            for j, want in enumerate(exp["palettes"]):
                self.same(f"palette of image {j} of the batch", bodies[j][:want.size].reshape(-1, 4), want)
                if not (bodies[j][want.size:] == PATTERN).all():
                    self.fail(f"palette of image {j} of the batch: written behind its out_counts entries")
            return
        if call == "b_reduce_indexed":
            self.same("out_counts of the batch", a["counts"].astype(np.int64), np.full(n, op[2], np.int64))
            for j, want in enumerate(exp["palettes"]):
                if not (a["pal_bufs"][j][4 * op[2]:] == PATTERN).all():
                    self.fail(f"palette of image {j} of the batch: written past the end")
                self.same(f"palette of image {j} of the batch", a["pal_bufs"][j][:4 * op[2]].reshape(-1, 4), want)
        for j, want in enumerate(exp["outputs"]):
            self.same(f"output of image {j} of {call} (mode {a['mode']}, format {a['fmt']}, cutoff {m.t})", self.typed(bodies[j], shapes[j], a["fmt"]), want)
        if call == "b_apply_device":
            self.sources_intact(imgs)

    def step_refuse_4(self, op, exp):
        env, m, what = self.env, self.model, op[1]
        if what == "batch_bad_tables":
            call, a = "b_apply_device", self.batch_args("b_apply_device", op[2], op[3], fmt=2, n_tables=op[4],
                                                         shared=int(op[4] <= 1 or op[4] > len(op[2])))
            if op[4] > 1:                                         # (tables enough for the count that is passed)
                a["c4"] = np.ascontiguousarray(np.stack(batch_tables(7, op[3], op[4], 0)), np.float32)
        elif what == "batch_empty":
            call = op[2]
            a = self.batch_args(call, (FLAT,), 4, fmt=int(call in ("b_reduce_indexed", "b_find", "b_apply_device")), n_images=0)
        else:
            call, imgs, k = op[2:5]
            kw = {}
            if what == "batch_no_kept_pixel":
                kw["bound"] = op[5]
                self.counters[f"batch_no_kept_pixel:bound_{op[5]}"] += 1
            if call != "b_palette_device" and call != "b_palette":
                kw["fmt"] = 1 if what == "batch_index8_full" else op[5] if what == "batch_meld_indexed" else 0
                kw["mode"] = 2 if what == "batch_meld_indexed" else 0
                if call == "b_reduce":
                    kw["fmt"] = 0
            self.counters[f"{what}:{call}"] += 1
            a = self.batch_args(call, imgs, k, **kw)
        status, message = env.batch(self.proc, a)
        env.sync()
        if status == 0:
            self.fail(f"a batched call the header refuses with status {exp['status']} was accepted")
        if status != exp["status"]:
            self.fail(f"refused with status {status}, the header names {exp['status']}")
        for needle in BATCH_NEEDLES[what] + ((exp["needle"],) if "needle" in exp else ()):
            if needle not in message:
                self.fail(f"the message of the refusal does not say {needle!r}: {message!r}")
        self.batch_untouched(a)

    # -- surface 2
    def step_refuse_2(self, op, st):
        m, proc, env, what = self.model, self.proc, self.env, op[1]
        if what in ("shared_frame_on_local", "local_frame_on_shared", "local_frame_no_output", "local_tolerance_without_delta", "warm_with_fixed"):
            q, img = self.seqs[op[2]], self.images[op[3]][1]
            if what == "shared_frame_on_local":
                self.expect_status(st, q.frame, img, delta=True)
            elif what == "local_tolerance_without_delta":
                self.expect_status(st, q.frame_local, img, delta=False, tolerance=40)
            else:
                self.counters["failed_frame:fixed_on_warm"] += int(what == "warm_with_fixed")
                self.expect_status(st, q.frame_local, img, delta=True)
        elif what in ("local_meld", "local_index8_k256"):
            self.coded[op[2]], self.remapped[op[2]] = [], {}
            self.expect_status(st, self.seqs[op[2]].output_local, op[3], 2 if what == "local_meld" else 0, 1, 96, 72)
        elif what in ("plan_indices_above_k", "plan_empty_record"):
            u = m.urec[op[2]]
            use = np.zeros(u["k"] + 2, np.uint64)
            if what == "plan_indices_above_k":
                use[:] = u["counts"]
                use[-1] += 1
            self.expect_status(st, env.index_plan, use, u["palette"], 0)
        elif what == "optimize_bits_too_narrow":
            pal, idx = proc.reduce_indexed(op[3], self.images[op[2]][1], 0, 0)
            self.expect_status(st, proc.optimize_indexed, idx, pal, index_ref.KEEP_UNUSED, 1)
        elif what == "remap_bad_bits":
            h, w = self.images[op[2]][1].shape[:2]
            self.arm(self.out2, 2 * w * h)
            self.expect_status(st, proc.index_remap_device, self.pix[op[2]].ptr, 1, w, h, 5, np.zeros(6, np.uint16), op[3], self.out2.ptr, self.bad.ptr,
                               env.streams[0])
            env.sync()
            if not (self.collect(self.out2, 2 * w * h, np.uint8, "refused call") == PATTERN).all():
                self.fail("a refused call wrote output")
        else:
            raise ValueError(op)

    def step_cpair(self, op, exp):
        env, proc, C, m = self.env, self.proc, self.counters, self.model
        P = op[1]
        pr = m.cpairs[P]
        fmt, k, offs = pr["fmt"], pr["k"], pr["offs"]
        h, w = pr["shown"].shape
        n, dt = w * h, index_dtype(fmt)
        sizes = {"index": fmt * n, "delta": fmt * n, "palette": 4 * k, "shown": 4 * n, "held": 4 * n}
        if op[0] == "cpair_open":
            self.count_k(k, fmt)
            # every buffer `offs` elements into a sentinel-filled allocation: offsets 0 and 4 allow the vector route, 1 does not
            bufs = {b: self.mem.alloc(offs * (fmt if b in ("index", "delta") else 4) + nb + GUARD) for b, nb in sizes.items()}
            bufs["rec"] = self.mem.alloc(48 + GUARD)
            self.mem.fill(bufs["rec"], 0, 48 + GUARD, PATTERN)
            for b, nb in sizes.items():
                self.mem.fill(bufs[b], 0, offs * (fmt if b in ("index", "delta") else 4) + nb + GUARD, PATTERN)
            for b in ("shown", "held"):
                self.mem.write(bufs[b], 4 * offs, np.zeros(4 * n, np.uint8))
            self.cpairs[P] = bufs
            return
        i, pseed, tol, nb, order, s = op[2:8]
        bufs = self.cpairs[P]
        off = {b: offs * (fmt if b in ("index", "delta") else 4) for b in sizes}
        ptr = {b: bufs[b].ptr + off[b] for b in sizes}
        C["cpair_exact" if tol is None else "cpair_lossy"] += 1
        C["route:per_pixel" if offs % 4 else "route:vector"] += 1
        self.arm(self.out, fmt * n)
        proc.apply(self.pix[i].ptr, w, h, 0, m.ref.find_centroids(exp["base"]), pseed % 2, self.out.ptr, env.streams[s], format=fmt)
        env.sync()
        index = self.collect(self.out, fmt * n, dt, "index map")
        self.same("index map of the frame", index.astype(np.int64).reshape(h, w), exp["index"])
        self.mem.write(bufs["index"], off["index"], index)
        self.mem.write(bufs["palette"], off["palette"], exp["palette"].reshape(-1))
        self.mem.fill(bufs["delta"], off["delta"], fmt * n, PATTERN)
        self.mem.write(bufs["rec"], 0, np.frombuffer(env.fresh_hold(), np.uint8).copy())
        bands = bands_of(h, nb, order)
        C[f"cdelta_bands:{len(bands)}"] += 1
        for j, (r0, rows) in enumerate(bands):
            a, e = 4 * r0 * w, fmt * r0 * w
            stj = env.streams[(s + j) % 2]
            if tol is None:
                proc.frame_delta_colour(ptr["index"] + e, ptr["palette"], ptr["shown"] + a, w, rows, r0, fmt, k, ptr["delta"] + e, bufs["rec"].ptr, stj)
            else:
                proc.frame_delta_colour_lossy(self.pix[i].ptr + a, ptr["index"] + e, ptr["palette"], ptr["shown"] + a, ptr["held"] + a, w, rows, r0, fmt, k,
                                              tol, ptr["delta"] + e, bufs["rec"].ptr, stj)
        env.sync()
        if tol is None:
            self.mem.write(bufs["held"], off["held"], self.images[i][1].reshape(-1))     # the caller's duty after an exact frame
        raw = self.collect(bufs["rec"], 48, np.uint8, "frame record")
        got = tuple(int(v) for v in raw[:16].view(np.uint64)) + tuple(int(v) for v in raw[16:32].view(np.uint32)) + \
            tuple(int(v) for v in raw[32:48].view(np.uint64))
        self.same("record of the colour-keyed frame", got, exp["record"])
        data = {}
        for b, nbytes in sizes.items():
            raw = self.mem.read(bufs[b], 0, off[b] + nbytes + GUARD)
            if not ((raw[:off[b]] == PATTERN).all() and (raw[off[b] + nbytes:] == PATTERN).all()):
                self.fail(f"{b}: written outside the buffer")
            data[b] = raw[off[b]:off[b] + nbytes].copy()
        self.same("delta map (colour-keyed)", data["delta"].view(dt).astype(np.int64).reshape(h, w), exp["delta"])
        self.same("shown canvas", data["shown"].view(np.uint32).reshape(h, w), exp["shown"])
        self.same("held source (colour-keyed)", data["held"].reshape(h, w, 4), exp["held"])
        self.same("index map after the pass", data["index"].view(dt), index)
        self.same("palette after the pass", data["palette"], exp["palette"].reshape(-1))

    def device_map(self, op, exp, t0):
        """the map of usage_device / remap_device, made on the device by the output pass into self.out"""
        env = self.env
        i, mode, fmt, k = op[1:5]
        h, w = self.images[i][1].shape[:2]
        self.arm(self.out, fmt * w * h)
        self.proc.apply(self.pix[i].ptr, w, h, 0, exp["cent"], mode, self.out.ptr, env.streams[op[-2] if op[0] == "usage_device" else op[-1]], format=fmt)
        env.sync()
        self.check_output(f"the map {op[0]} works on (mode {mode}, format {fmt}, cutoff {t0})", fmt, w, h, exp["index"])
        return w, h

    def step_index(self, op, exp, t0):
        env, proc, C, m, name = self.env, self.proc, self.counters, self.model, op[0]
        if name == "usage_device":
            fmt, k, rec, nb, order, s, fresh = op[3], op[4], op[6], op[7], op[8], op[9], op[10]
            C[f"usage:{ {1: 'index8', 2: 'index16'}[fmt] }:{k_class(k)}"] += 1
            C["usage_fresh" if fresh else "usage_combined_across_images"] += 1
            w, h = self.device_map(op, exp, t0)
            if fresh:
                self.new_record(rec, k)
            bands = bands_of(h, nb, order)
            C[f"usage_bands:{len(bands)}"] += 1
            for j, (r0, rows) in enumerate(bands):
                proc.index_usage_device(self.out.ptr + fmt * r0 * w, rows * w, fmt, k, self.urec[rec].ptr, env.streams[(s + j) % 2])
            env.sync()
            self.same("usage record", self.read_record(rec, k), exp["counts"])
        elif name == "plan":
            rec, slot, flags = op[1:4]
            C[f"plan_order:{flags & 3}"] += 1
            for bit in (4, 8, 16):
                C[f"plan_flag:{bit}"] += int(bool(flags & bit))
            k = m.urec[rec]["k"]
            use = self.read_record(rec, k)
            self.same("the record the plan is made from", use, exp["counts"])
            remap, pal, info = env.index_plan(use, exp["source"], flags)
            self.same("remap table of the plan", remap, exp["remap"])
            self.same("palette of the plan", pal, exp["palette"])
            self.same("info of the plan", tuple(info), exp["info"])
        elif name == "remap_device":
            fmt, k, table, bits, in_place, bad_fresh, s = op[3], op[4], op[6], op[7], op[8], op[9], op[10]
            C[f"remap_bits:{bits}"] += 1
            C["remap_planned_table" if isinstance(table, int) else "remap_random_table"] += 1
            C["remap_in_place"] += int(in_place)
            C["bad_count_combined"] += int(not bad_fresh)
            w, h = self.device_map(op, exp, t0)
            nbytes = exp["out"].nbytes
            dst = self.out if in_place else self.out2
            if not in_place:
                self.arm(self.out2, nbytes)
            if bad_fresh:
                self.mem.write(self.bad, 0, np.zeros(8, np.uint8))
            proc.index_remap_device(self.out.ptr, fmt, w, h, k, exp["table"], bits, dst.ptr, self.bad.ptr, env.streams[s])
            env.sync()
            self.same(f"remapped map at {bits} bits", self.collect(dst, nbytes, exp["out"].dtype, "remapped map").reshape(exp["out"].shape), exp["out"])
            got = int(self.collect(self.bad, 8, np.uint64, "bad count")[0])
            if got != exp["bad"]:
                self.fail(f"bad-pixel count {got}, the model {exp['bad']}")
            if not in_place:
                self.check_output("the input map after the remap", fmt, w, h, exp["index"])
        elif name == "optimize":
            i, k, mode, flags, bits = op[1:6]
            self.count_k(k, host_format(k, t0))
            C["optimize_plan_bits" if bits == 0 else "optimize_given_bits"] += 1
            pal, idx = proc.reduce_indexed(k, self.images[i][1], 0, mode)
            self.same("palette of reduce_indexed", pal, exp["source"])
            self.same("index map of reduce_indexed", idx.astype(np.int64), exp["index"])
            out_pal, out, info = proc.optimize_indexed(idx, pal, flags, bits or None)
            self.same("info of optimize", tuple(info.as_tuple()), exp["info"])
            self.same("palette of optimize", out_pal, exp["palette"])
            self.same(f"map of optimize at {exp['bits']} bits", out, exp["out"])
        else:
            raise ValueError(op)


def run_sequence(env, seed, seq, ops=None, counters=None, proc=None, cache=None, surface=1):
    """one sequence on a fresh processor (or the caller's): (ops run, blocks allocated, blocks re-used); raises Mismatch with the
    replay text"""
    ops = generate(seed, seq, surface=surface) if ops is None else ops
    r = Runner(env, seed, seq, counters, proc, cache)
    try:
        before = r.proc.debug_block_counts()
        r.run(ops)
        blocks = r.proc.debug_block_counts()
    except Mismatch as e:
        raise Mismatch(f"seed {seed} sequence {seq}: {e}\nreplay(env, {seed}, {seq}, {ops[:r.n_ops + 1]!r})") from None
    finally:
        r.close()
    return r.n_ops, blocks[0] - before[0], blocks[1] - before[1]


def replay(env, seed, seq, ops, proc=None):
    """runs a printed op list again: the images are those of (seed, seq)"""
    return run_sequence(env, seed, seq, ops, proc=proc)


# ---- the real binding -----------------------------------------------------------------------------------------------
class KgEnv(LH.KgEnv):
    """lifecycle_harness.KgEnv with the processor of this harness: the shrink of the palette step stays on"""

    def session_processor(self):
        return self.kg.ImageProcessor(shrink_max_dim=SHRINK, max_iterations=MAX_ITERATIONS, check_period=CHECK_PERIOD, strategy="auto")

    def index_plan(self, usage, palette, flags):
        remap, pal, info = self.kg.index_plan(usage, palette, flags)
        return remap, pal, info.as_tuple()

    def set_weighting(self, proc, value):
        """kmg_processor_set_weighting with any value (ImageProcessor.set_alpha_weight passes the two legal ones only)"""
        self.kg._check(self.kg.lib().kmg_processor_set_weighting(proc.handle, int(value)))

    def fresh_hold(self):
        return self.kg.FrameHold.fresh_bytes()

    def batch(self, proc, a):
        """one batched call of the C ABI on the arguments Runner.batch_args made: (status, message of kmg_last_error)"""
        import ctypes as C
        kg, L, n = self.kg, self.kg.lib(), len(a["src"])
        vp, u32 = C.c_void_p, C.c_uint32
        src, ws, hs = (vp * n)(*a["src"]), (u32 * n)(*a["ws"]), (u32 * n)(*a["hs"])
        out = (vp * n)(*a["out"]) if "out" in a else None
        rep = C.cast(a["rep"].ctypes.data, C.POINTER(kg.BatchReport))
        arep = C.cast(a["arep"].ctypes.data, C.POINTER(kg.BatchApplyReport))

        def ptr(name, ctype):
            return a[name].ctypes.data_as(C.POINTER(ctype))
        call, h = a["call"], proc.handle
        if call == "b_palette":
            rc = L.kmg_palette_batch(h, a["n"], src, ws, hs, a["k"], a["algo"], a["bound"], out, ptr("counts", u32), rep)
        elif call == "b_reduce":
            rc = L.kmg_reduce_batch(h, a["n"], src, ws, hs, a["k"], a["algo"], a["mode"], a["bound"], out, rep)
        elif call == "b_reduce_indexed":
            rc = L.kmg_reduce_indexed_batch(h, a["n"], src, ws, hs, a["k"], a["algo"], a["mode"], a["fmt"], a["bound"], (vp * n)(*a["pal_out"]),
                                            ptr("counts", u32), out, rep, arep)
        elif call == "b_find":
            rc = L.kmg_find_batch(h, a["n"], src, ws, hs, ptr("palette", C.c_uint8), a["k"], a["mode"], a["fmt"], a["bound"], out, arep)
        elif call == "b_palette_device":
            rc = L.kmg_dev_palette_batch(h, a["n"], src, ws, hs, a["k"], ptr("cent", C.c_float), ptr("its", u32), rep, vp(a["stream"]))
        else:
            rc = L.kmg_dev_apply_batch(h, a["n"], src, ws, hs, ptr("c4", C.c_float), a["n_tables"], a["k"], a["mode"], a["fmt"], out, arep,
                                       vp(a["stream"]))
        return rc, L.kmg_last_error().decode() if rc else ""
