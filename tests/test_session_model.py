"""tests/session_harness.py shown to be SOUND and SHARP on the CPU, before the device sees it (tests/test_gpu_session.py runs the
same seeds; the generator is deterministic, so what is covered here is covered there).

Sound: stand-ins of kmeans_gpu_amd.ImageProcessor / Sequence / Lloyd / ApplyPlan over the reference modules, which keep the state
the library keeps -- the sticky switches and the moment each consumer reads them, the working sequence as compacted pixels in a
block that grows geometrically, the first-frame record, canvas and held source of an open output in a block that goes back to the
idle list, n_fixed with the object -- pass every sequence of every committed seed.  Sharp: thirteen faulty variants, one named
defect each, are each caught by every committed seed.  Coverage: exact counts for the committed seeds, none zero.

Surface 2 (per-frame palettes, colour-keyed canvases, index-map optimisation) has seeds of its own, SEEDS_2, whose sequences also
run the old ops: the stand-ins keep shown, held source and the last centroids of a local output where the library keeps them (shown
filled at the begin, the held source not; the centroids in the sequence), usage records and the bad count combine; thirteen more
faulty variants, and the thirteen old ones, are each caught by each of SEEDS_2; a second exact table, EXACT_2.  The op lists of the
old seeds are pinned by hash: surface 2 must not move them.

Surface 3 (alpha weighting on the processor and on the Lloyd objects) has SEEDS_3: the stand-ins keep the processor's switch, read
it where the library reads it (the cutoff of a working image where the image is made, the loop where it starts), keep a Lloyd
object's weighting and both kinds of binding; twelve more faulty variants, and the twenty-six old ones, are each caught by each of
SEEDS_3; a third exact table, EXACT_3.  The op lists of SEEDS_2 and the fourteen old images are pinned by hash as well.

Surface 4 (the batched calls) has SEEDS_4: the stand-ins gain the six batched calls, built from the per-image stand-ins -- what a
batch adds is where a result goes (its index in the caller's arrays, through the sub-batches), when the switches are read (at the
call), what is refused before anything is written, and the state of a chain of batched launches in a block of the idle list (the
results come back by slot).  Nine faulty variants, FAULTS_4, are each caught by each of SEEDS_4; a fourth exact table, EXACT_4.  The
sequences of surface 4 hold fewer of the older directed passages (so that a seed costs what the other seeds cost), so the older
faulty variants stay with the campaigns of their own surfaces.  The op lists of SEEDS_3, and those of SEEDS_4, are pinned by hash.

Wall time of this file and of tests/test_lifecycle_model.py: profiles/NOTES.md, "session harness"."""
import collections
import hashlib

import numpy as np
import pytest

import session_harness as H
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
from lifecycle_harness import sorted_palette
from test_lifecycle_model import FakeError, HostMem, _view

SEEDS = (201, 202)          # the seeds tests/test_gpu_session.py runs
SEQUENCES = 6               # ... and its sequences per seed

FAULTS = ("cutoff_read_at_palette_time", "plan_follows_cutoff", "fixed_sticks_after_none", "n_fixed_inherited", "set_fixed_zero_ignored",
          "canvas_survives_end_output", "held_not_reanchored", "held_frame_swap_lost", "record_not_reset", "band_combined_twice",
          "clear_keeps_first_frame", "w_growth_drops_tail", "quality_leaves_switch")


# surface 2 (per-frame palettes, colour-keyed canvases, index-map optimisation): its own seeds, which also run every old op
SEEDS_2 = (314, 315)
FAULTS_2 = ("warm_after_failed_frame", "warm_survives_begin", "shown_survives_begin", "failed_frame_touches_shown",
            "local_switches_read_at_begin", "held_not_reanchored_local", "lossy_full_keeps_lossy_canvas", "duplicate_entries_sent",
            "usage_overwrites", "usage_index8_256_touches_tail", "bad_count_overwrites", "optimize_counts_leak", "remap_padding_dirty")


# surface 3 (alpha weighting on the processor and on the Lloyd objects): its own seeds, which also run every op of surfaces 1 and 2
SEEDS_3 = (421, 422)
# weight_set_under_binding can be caught only through the refusal l_weight_under_caller_binding: the deviation is that a call the
# header refuses is accepted, and the generator never emits that call but as a listed refusal (warm_after_failed_frame is the
# precedent: there the refusal is what moves the state).
FAULTS_3 = ("weight_read_at_add", "add_cutoff_ignores_weight", "output_cutoff_follows_weight", "weight_off_ignored", "bad_value_clears_weight",
            "lloyd_weight_inherited", "weighted_object_uses_binding", "weight_set_under_binding", "warm_frame_unweighted", "init_weighted",
            "quality_record_weighted", "zero_weight_cluster_counts_pixels")
NEW_OPS_3 = ("weight", "l_weight", "l_unbind", "motif")


# surface 4 (the batched calls): its own seeds, which also run every op of surfaces 1 to 3
SEEDS_4 = (533, 534)
FAULTS_4 = ("stale_stop_word", "second_sub_batch_indexes_from_0", "per_image_tables_read_table_0", "batch_cutoff_read_once",
            "find_batch_refuses_fixed", "batch_weight_refusal_sticks", "refused_batch_writes_first_sub_batch", "out_counts_unwritten",
            "iterations_of_last_image")
NEW_OPS_4 = H.BATCH_OPS


NEW_OPS = ("s_output_local", "s_frame_local", "cpair_open", "cpair_frame", "usage_device", "plan", "remap_device", "optimize", "s_usage",
           "s_remap")


class Record:
    def __init__(self, values):
        self.values = tuple(int(v) for v in values)

    def as_tuple(self):
        return self.values


def _record_view(ptr, lossy):
    """the integers of a kmg_frame_delta / kmg_frame_hold in device memory, and a function that writes them back"""
    raw = _view(ptr, 48 if lossy else 32, np.uint8)
    vals = [int(v) for v in raw[:16].view(np.uint64)] + [int(v) for v in raw[16:32].view(np.uint32)]
    if lossy:
        vals += [int(v) for v in raw[32:48].view(np.uint64)]

    def put(rec):
        raw[:16] = np.array(rec[:2], np.uint64).view(np.uint8)
        raw[16:32] = np.array(rec[2:6], np.uint32).view(np.uint8)
        if lossy:
            raw[32:48] = np.array(rec[6:8], np.uint64).view(np.uint8)
    return tuple(vals), put


class FakeProcessor:
    def __init__(self, fault, images, cache):
        self.fault = fault
        self.ref = H.Ref(images, cache)
        self.by_bytes = {a.tobytes(): i for i, (_, a) in enumerate(images)}
        self.t, self.fixed, self.strategy = 0, None, 0
        self.w = 0                     # kmg_processor_set_weighting
        self.idle = []                 # blocks of closed objects and ended outputs: what their last owner left in them
        self.allocated = self.reused = 0
        self.last_compare = error_ref.ZERO
        self.opt_counts = None
        self.batch_t = None            # (a faulty variant's: the cutoff of the first batched call)
        self.weight_refused = False    # (a faulty variant's: a batch was refused for the weighting)

    # -- blocks
    def take(self):
        if self.idle:
            self.reused += 1
            return self.idle.pop()
        self.allocated += 1
        return {}

    def give(self, block):
        self.idle.append(block)

    def scratch(self):
        self.give(self.take())

    def debug_block_counts(self):
        return self.allocated, self.reused

    def close(self):
        pass

    # -- switches
    def set_alpha_cutoff(self, t):
        self.t = int(t)

    def set_fixed_colors(self, colors):
        if colors is None or len(colors) == 0:
            if self.fault != "fixed_sticks_after_none":
                self.fixed = None
            return
        self.fixed = tuple(tuple(int(v) for v in c) for c in np.asarray(colors, np.uint8))

    def set_strategy(self, v):
        self.strategy = int(v)

    def set_weighting(self, v):
        if v not in (0, 1):
            if self.fault == "bad_value_clears_weight":
                self.w = 0
            raise FakeError(-1, "unknown weighting")
        if v == 0 and self.fault == "weight_off_ignored":
            return
        self.w = int(v)

    def set_alpha_weight(self, on):
        self.set_weighting(1 if on else 0)

    def wc(self):
        """the cutoff of a working image made now"""
        return max(self.t, 1) if self.w else self.t

    def out_t(self):
        """the cutoff of an output made now: t, whatever the weighting"""
        return 1 if self.fault == "output_cutoff_follows_weight" and self.w and self.t == 0 else self.t

    def fid(self):
        return H.FIXED.index(self.fixed)

    def n_fixed(self):
        return 0 if self.fixed is None else len(self.fixed)

    def image_index(self, a):
        return self.by_bytes[np.ascontiguousarray(a).tobytes()]

    # -- the palette step of a host call: the switches as they are when it starts
    def _centroids(self, image, k, algo=0):
        f = self.n_fixed()
        if algo == 1 and (f or self.w):
            raise FakeError(-1, "the octree has no fixed colours and no weighting")
        if k < f:
            raise FakeError(-1, "k is below the fixed colours")
        i = self.image_index(image)
        if self.ref.working(((i, self.wc()),)) is None:
            raise FakeError(-1, "no pixel reaches alpha_cutoff")
        self.scratch()
        if self.fault == "init_weighted" and self.w and self.t == 0:
            # the initialisation on the pixels kept at t, the weighted loop on those kept at max(t, 1)
            W0, w0, h0 = self.ref.working(((i, 0),))
            W1 = self.ref.working(((i, 1),))[0]
            pins = fixed_ref.pins_lab(O, () if self.fixed is None else np.array(self.fixed, np.uint8))
            cent0 = fixed_ref.init_centroids(O, O.rgb_to_lab(W0), w0, h0, k, pins) if f else O.init_centroids(O.rgb_to_lab(W0), w0, h0, k)
            return weight_ref.lloyd(O, O.rgb_to_lab(W1), W1[:, 3], cent0, f, H.MAX_ITERATIONS, H.CHECK_PERIOD)[0]
        return self.ref.centroids(((i, self.wc()),), k, self.fid(), self.w)

    def palette(self, k, image, algo=0):
        return sorted_palette(self._centroids(image, k, algo))

    def reduce(self, k, image, algo=0, reduce_mode=0, out=None):
        res = self.ref.rgba(image, self._centroids(image, k, algo), reduce_mode, self.out_t())
        if out is not None:
            out[:] = res
        return res

    def _typed(self, idx, k, t):
        return idx.astype(H.index_dtype(H.host_format(k, t)))

    def reduce_indexed(self, k, image, algo=0, reduce_mode=0):
        cent = self._centroids(image, k, algo)
        return self.ref.palette_bytes(cent), self._typed(self.ref.index(image, cent, reduce_mode, self.out_t()), k, self.t)

    def find(self, image, colors, reduce_mode=0):
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        if self.t:
            return alpha_ref.find(O, image, pal, reduce_mode, self.t)
        if reduce_mode == 3:
            return diffuse_ref.diffuse(image, diffuse_ref.oracle_find_replace(O, pal))
        return O.find(image, pal, reduce_mode)

    def find_indexed(self, image, colors, reduce_mode=0):
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        return self._typed(self.ref.index(image, self.ref.find_centroids(pal), reduce_mode, self.t), pal.shape[0], self.t)

    def compare(self, src, out, palette=None, what=3):
        rec = self.ref.stats(src, np.asarray(out).astype(np.int64) if palette is not None else out, palette, self.t, what)
        if self.fault == "record_not_reset":
            rec = error_ref.combine(self.last_compare, rec)
        self.last_compare = rec
        return Record(rec)

    def reduce_quality(self, image, max_delta_e, k_min=2, k_max=256, reduce_mode=0, indexed=False):
        if k_min < self.n_fixed():
            raise FakeError(-1, "k_min is below the fixed colours")
        i, t = self.image_index(image), self.t
        self.scratch()
        k, reached, rec = self.ref.quality(i, self.wc(), self.fid(), H.target_of(max_delta_e), k_min, k_max, self.w)
        cent = self.ref.centroids(((i, self.wc()),), k, self.fid(), self.w)
        if self.fault == "quality_record_weighted" and self.w:       # the record of the list in which pixel i appears a_i times
            W = self.ref.working(((i, self.wc()),))[0]
            rep = np.ascontiguousarray(np.repeat(W, W[:, 3].astype(np.int64), axis=0))
            rec = error_ref.stats(O, rep, O.assign(O.rgb_to_lab(rep), cent), palette=self.ref.palette_bytes(cent))
        out = self._typed(self.ref.index(image, cent, reduce_mode, t), k_max, t) if indexed else self.ref.rgba(image, cent, reduce_mode, t)
        if self.fault == "quality_leaves_switch":
            self.t = 0 if t else 255               # the bisection's own setting is left behind
        return k, self.ref.palette_bytes(cent), out, Record(rec), reached

    # -- device calls
    def _check_format(self, k, mode, fmt, t):
        if fmt in (1, 2) and mode == 2:
            raise FakeError(-1, "meld has no index output")
        if fmt == 1 and k + (1 if t else 0) > 256:
            raise FakeError(-1, "INDEX8 holds 256 indices")

    def _pass(self, img, cent, mode, fmt, t):
        return self.ref.rgba(img, cent, mode, t) if fmt is None else self.ref.index(img, cent, mode, t)

    def _write(self, d_out, a, fmt):
        a = np.ascontiguousarray(a)
        _view(d_out, a.size, np.uint8 if fmt is None else H.index_dtype(fmt))[:] = a.reshape(-1)

    def apply(self, d_rgba, width, rows, row0, cent, mode, d_out, stream=0, format=None):
        cent = np.ascontiguousarray(cent, np.float32).reshape(-1, 4)
        self._check_format(cent.shape[0], mode, format, self.t)
        self.scratch()
        assert row0 == 0
        img = _view(d_rgba, 4 * width * rows, np.uint8).reshape(rows, width, 4)
        self._write(d_out, self._pass(img, cent, mode, format, self.t), format)

    def apply_plan(self, cent, mode, n_pixels_hint, stream=0, format=None):
        proc = self
        cent = np.ascontiguousarray(cent, np.float32).reshape(-1, 4).copy()
        self._check_format(cent.shape[0], mode, format, self.t)
        block = self.take()
        made_under = self.t

        class Plan:
            def __init__(self):
                self.bands = []

            def run(self, d_rgba, width, rows, row0, d_out, stream=0):
                # (the bands of a sequence tile one image from row 0: Bayer coordinates and the diffusion continue across them)
                self.bands.append(_view(d_rgba, 4 * width * rows, np.uint8).reshape(rows, width, 4).copy())
                t = proc.t if proc.fault == "plan_follows_cutoff" else made_under
                whole = proc._pass(np.ascontiguousarray(np.concatenate(self.bands)), cent, mode, format, t)
                proc._write(d_out, whole[row0:row0 + rows], format)

            def status(self):
                pass

            def close(self):
                proc.give(block)
        return Plan()

    def alpha_compact(self, d_rgba, n_pixels, cutoff, d_out, d_n_kept, stream=0):
        kept = alpha_ref.compact(_view(d_rgba, 4 * n_pixels, np.uint8).reshape(-1, 4), cutoff)
        _view(d_out, kept.size, np.uint8)[:] = kept.reshape(-1)
        _view(d_n_kept, 1, np.uint64)[0] = kept.shape[0]

    def compare_device(self, d_src, d_out, n_pixels, d_stats, format=0, palette=None, alpha_cutoff=0, what=3, stream=0):
        if format == 1 and palette is not None and len(palette) + (1 if alpha_cutoff else 0) > 256:
            raise FakeError(-1, "INDEX8 holds 256 indices")
        src = _view(d_src, 4 * n_pixels, np.uint8).reshape(-1, 4)
        out = _view(d_out, 4 * n_pixels, np.uint8).reshape(-1, 4) if format == 0 else _view(d_out, n_pixels, H.index_dtype(format)).astype(np.int64)
        rec = self.ref.stats(src, out, palette, alpha_cutoff, what)
        stats = _view(d_stats, 14, np.uint64)
        for _ in range(2 if self.fault == "band_combined_twice" else 1):
            stats[:] = np.array(error_ref.combine(tuple(int(v) for v in stats), rec), np.uint64)

    def _band(self, ptr, width, rows, fmt):
        return _view(ptr, width * rows, H.index_dtype(fmt)).reshape(rows, width)

    def frame_delta(self, d_index, d_canvas, width, rows, row0, format, k, d_delta, d_info, stream=0):
        index, canvas = self._band(d_index, width, rows, format), self._band(d_canvas, width, rows, format)
        d, new_canvas, rec = sequence_ref.delta(index.astype(np.int64), canvas.astype(np.int64), k, row0)
        self._band(d_delta, width, rows, format)[:] = d
        canvas[:] = new_canvas
        old, put = _record_view(d_info, False)
        for _ in range(2 if self.fault == "band_combined_twice" else 1):
            old = sequence_ref.combine(old, rec)
        put(old)

    def frame_delta_lossy(self, d_src, d_index, d_canvas, d_held, width, rows, row0, format, k, tolerance, d_delta, d_info, stream=0):
        index, canvas = self._band(d_index, width, rows, format), self._band(d_canvas, width, rows, format)
        src = _view(d_src, 4 * width * rows, np.uint8).reshape(rows, width, 4)
        held = _view(d_held, 4 * width * rows, np.uint8).reshape(rows, width, 4)
        d, new_canvas, new_held, rec = hold_ref.hold(O, src, index.astype(np.int64), canvas.astype(np.int64), held, k, tolerance, row0)
        if self.fault == "held_not_reanchored":
            new_held = np.where((canvas.astype(np.int64) != k)[..., None], held, new_held)
        self._band(d_delta, width, rows, format)[:] = d
        canvas[:] = new_canvas
        held[:] = new_held
        old, put = _record_view(d_info, True)
        for _ in range(2 if self.fault == "band_combined_twice" else 1):
            old = hold_ref.combine(old, rec)
        put(old)

    # -- colour-keyed delta passes on the caller's canvas
    def _colour_band(self, d_index, d_palette, d_shown, width, rows, format, k):
        return (self._band(d_index, width, rows, format).astype(np.int64), _view(d_palette, 4 * k, np.uint8).reshape(k, 4),
                _view(d_shown, width * rows, np.uint32).reshape(rows, width))

    def frame_delta_colour(self, d_index, d_palette, d_shown, width, rows, row0, format, k, d_delta, d_info, stream=0):
        index, pal, shown = self._colour_band(d_index, d_palette, d_shown, width, rows, format, k)
        d, new_shown, rec = local_ref.colour(index, shown, pal, k, row0)
        if self.fault == "duplicate_entries_sent":                       # entries are told apart by index: a repeat of an earlier entry is "another colour"
            c, p = local_ref.lookup(index, pal, k)
            table = np.concatenate([local_ref.words(pal), np.zeros(1, np.uint32)])
            first = np.array([int(np.flatnonzero(table == w)[0]) for w in table])
            ch = (p != shown) | (first[c] != c)
            d, rec = np.where(ch, c, k), local_ref._record(ch, p, row0)
        self._band(d_delta, width, rows, format)[:] = d
        shown[:] = new_shown
        old, put = _record_view(d_info, False)
        put(local_ref.combine(old, rec))

    def frame_delta_colour_lossy(self, d_src, d_index, d_palette, d_shown, d_held, width, rows, row0, format, k, tolerance, d_delta, d_info,
                                 stream=0):
        index, pal, shown = self._colour_band(d_index, d_palette, d_shown, width, rows, format, k)
        src = _view(d_src, 4 * width * rows, np.uint8).reshape(rows, width, 4)
        held = _view(d_held, 4 * width * rows, np.uint8).reshape(rows, width, 4)
        d, new_shown, new_held, rec = local_ref.lossy(O, src, index, shown, held, pal, k, tolerance, row0)
        self._band(d_delta, width, rows, format)[:] = d
        shown[:] = new_shown
        held[:] = new_held
        old, put = _record_view(d_info, True)
        put(local_ref.combine(old, rec))

    # -- index-map optimisation
    def _check_index(self, format, k, n):
        if format not in (1, 2) or k == 0 or k > index_ref.MAX_K or (format == 1 and k > 256) or n == 0:
            raise FakeError(-1, "index format, k or size")

    def _count(self, index, k, use, format):
        counts = index_ref.usage(index, k)
        if self.fault == "usage_index8_256_touches_tail" and format == 1 and k == 256:
            counts[256] = counts[0]                                      # the byte 0 taken for slot 256
        use[:] = counts if self.fault == "usage_overwrites" else use + counts

    def index_usage_device(self, d_index, n_pixels, format, k, d_usage, stream=0):
        self._check_index(format, k, n_pixels)
        self._count(_view(d_index, n_pixels, H.index_dtype(format)), k, _view(d_usage, k + 2, np.uint64), format)

    def _remap(self, a, k, remap, bits):
        new, bad = index_ref.remap_fast(a, k, remap, bits)
        out = index_ref.pack_fast(new, bits)
        if self.fault == "remap_padding_dirty" and bits < 8 and (a.shape[1] * bits) % 8:
            out[:, -1] |= 1
        return out, bad

    def index_remap_device(self, d_in, in_format, width, rows, k, remap, out_bits, d_out, d_bad, stream=0):
        self._check_index(in_format, k, width * rows)
        if out_bits not in H.BITS:
            raise FakeError(-1, "out_bits")
        out, bad = self._remap(_view(d_in, width * rows, H.index_dtype(in_format)).reshape(rows, width).copy(), k, remap, out_bits)
        _view(d_out, out.size, out.dtype)[:] = out.reshape(-1)
        count = _view(d_bad, 1, np.uint64)
        count[0] = bad if self.fault == "bad_count_overwrites" else int(count[0]) + bad

    def index_usage(self, index, k, usage=None):
        a = np.ascontiguousarray(index)
        use = np.zeros(k + 2, np.uint64) if usage is None else usage
        self._check_index(1 if a.dtype == np.uint8 else 2, k, a.size)
        self._count(a, k, use, 1 if a.dtype == np.uint8 else 2)
        return use

    def index_remap(self, index, k, remap, bits):
        a = np.ascontiguousarray(index)
        self._check_index(1 if a.dtype == np.uint8 else 2, k, a.size)
        return self._remap(a, k, remap, bits)

    def optimize_indexed(self, index, palette, flags=17, bits=None):
        a = np.ascontiguousarray(index)
        pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
        k = pal.shape[0]
        counts = index_ref.usage(a, k)
        if self.fault == "optimize_counts_leak" and self.opt_counts is not None:     # the call's device record is not zeroed
            counts[:k + 1] += np.resize(self.opt_counts, k + 1)
        self.opt_counts = counts
        planned = index_ref.plan(counts, pal, flags)
        if planned is None:
            raise FakeError(-1, "the plan refuses")
        remap, out_pal, info = planned
        b = bits or info[3]
        if b < info[3] or b > 8 * a.dtype.itemsize:
            raise FakeError(-1, "out_bits")
        return out_pal, self._remap(a, k, remap, b)[0], Record(info)

    # -- the batched calls, from the per-image stand-ins: what a batch adds is where a result goes, when the switches are read, and
    # the state of a chain in a block of the idle list
    def _batch_images(self, a):
        if a["n"] == 0:
            raise FakeError(-1, "the batch is empty")
        return [_view(p, 4 * w * h, np.uint8).reshape(h, w, 4) for p, w, h in zip(a["src"], a["ws"], a["hs"])][:a["n"]]

    def _batch_t(self):
        """the cutoff of a batched call: the processor's, as it is when the call starts"""
        if self.fault == "batch_cutoff_read_once":
            self.batch_t = self.t if self.batch_t is None else self.batch_t
            return self.batch_t
        return self.t

    def _batch_refusals(self, a, t, palette_step):
        k, mode, fmt = a["k"], a["mode"], a["fmt"]
        if fmt in (1, 2) and mode == 2:
            raise FakeError(-1, "meld blends two colours: it has no index output")
        if fmt == 1 and k + (1 if t else 0) > 256:
            raise FakeError(-1, "INDEX8 holds 256 indices")
        if palette_step:
            if self.n_fixed():
                raise FakeError(-1, "a batch has no fixed colours")
            if self.w or (self.fault == "batch_weight_refusal_sticks" and self.weight_refused):
                self.weight_refused = True
                raise FakeError(-1, "a batch has no alpha weighting")

    def _put(self, a, at, data):
        """the bytes of a result into output `at`, as far as that output has room"""
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        nb = min(raw.size, a["room"][at])
        _view(a["out"][at], nb, np.uint8)[:] = raw[:nb]

    def _chain(self, results, k):
        """the batched kernels on one piece: its state lives in a block of the idle list, the results come back by slot"""
        block = self.take()
        stale = block.get("batch_cent")
        block["batch_cent"] = [c for c, _ in results]
        self.give(block)
        if self.fault == "stale_stop_word" and stale is not None and len(stale) > len(results):
            # the stop words of the block's last batch still stand: the slot's old centroid buffer is gathered
            out = []
            for q, (_, it) in enumerate(results):
                c = np.resize(stale[q], (k, 4)).astype(np.float32)
                c[:, 3] = 1.0
                out.append((c, it))
            return out
        return results

    def _find_rgba(self, img, pal, mode, t):
        if t:
            return alpha_ref.find(O, img, pal, mode, t)
        if mode == 3:
            return diffuse_ref.diffuse(img, diffuse_ref.oracle_find_replace(O, pal))
        return O.find(img, pal, mode)

    def _indexed(self, idx, fmt):
        return idx.astype(H.index_dtype(fmt))

    def _output_report(self, a, n, pieces, mode, algo=0):
        batched, per_image = H.batch_output_report(self, n, mode, algo)
        a["arep"][:] = (len(pieces) if batched else 0, batched, per_image, len(pieces))

    def _batch_host(self, a, call):
        imgs = self._batch_images(a)
        k, algo, mode, fmt = a["k"], a["algo"], a["mode"], a["fmt"]
        t = self._batch_t()
        self._batch_refusals(a, t, True)
        idx = [self.image_index(im) for im in imgs]
        pieces = H.batch_cut([H.batch_resident(im.shape[:2], t, call, fmt) for im in imgs], a["bound"])
        gone = [j for j, i in enumerate(idx) if self.ref.working(((i, t),)) is None]
        if gone and self.fault != "refused_batch_writes_first_sub_batch":
            raise FakeError(-1, f"image {gone[0]}: no pixel reaches alpha_cutoff = {t}")
        rep, its = [0, 0, len(pieces), 0], []
        for s, piece in enumerate(pieces):
            if set(piece) & set(gone):
                raise FakeError(-1, f"image {min(set(piece) & set(gone))}: no pixel reaches alpha_cutoff = {t}")
            if algo == 0:
                results = [self.ref.palette_step(idx[j], t, k) for j in piece]
                if len(piece) >= 2:
                    rep[0] += k + 2 + max(it for _, it in results)
                    results = self._chain(results, k)
                else:
                    self.scratch()                                   # a sub-batch of one image: the per-image palette step
                its += [it for _, it in results]
            for q, j in enumerate(piece):
                at = q if self.fault == "second_sub_batch_indexes_from_0" and s > 0 else j
                img = imgs[j]
                if algo == 1:
                    res = self.ref._memo(("octree", idx[j], k) + ((mode,) if call != "b_palette" else ()),
                                         lambda: O.palette_octree(img, k) if call == "b_palette" else O.reduce_octree(img, k, mode))
                    self._put(a, at, res)
                    count = res.shape[0]
                else:
                    cent, count = results[q][0], k
                    if call == "b_palette":
                        self._put(a, at, sorted_palette(cent))
                    elif call == "b_reduce" or fmt == 0:
                        self._put(a, at, self.ref.rgba(img, cent, mode, t))
                    else:
                        self._put(a, at, self._indexed(self.ref.index(img, cent, mode, t), fmt))
                    if call == "b_reduce_indexed":
                        _view(a["pal_out"][at], 4 * k, np.uint8)[:] = self.ref.palette_bytes(cent).reshape(-1)
                if call != "b_reduce" and self.fault != "out_counts_unwritten":
                    a["counts"][at] = count
            if call != "b_palette":
                self.scratch()                                       # the records and tables of the output step
        if its:
            rep[1] = its[-1] if self.fault == "iterations_of_last_image" else max(its)
        a["rep"][:] = rep
        if call == "b_reduce_indexed":
            self._output_report(a, len(imgs), pieces, mode, algo)

    def batch_palette(self, a):
        self._batch_host(a, "b_palette")

    def batch_reduce(self, a):
        self._batch_host(a, "b_reduce")

    def batch_reduce_indexed(self, a):
        self._batch_host(a, "b_reduce_indexed")

    def batch_find(self, a):
        imgs = self._batch_images(a)
        mode, fmt, pal = a["mode"], a["fmt"], a["palette"]
        t = self._batch_t()
        self._batch_refusals(a, t, False)
        if self.fault == "find_batch_refuses_fixed" and self.n_fixed():
            raise FakeError(-1, "a batch has no fixed colours")
        pieces = H.batch_cut([H.batch_resident(im.shape[:2], t, "b_find", fmt) for im in imgs], a["bound"])
        for s, piece in enumerate(pieces):
            self.scratch()
            for q, j in enumerate(piece):
                at = q if self.fault == "second_sub_batch_indexes_from_0" and s > 0 else j
                if fmt == 0:
                    self._put(a, at, self._find_rgba(imgs[j], pal, mode, t))
                else:
                    self._put(a, at, self._indexed(self.ref.index(imgs[j], self.ref.find_centroids(pal), mode, t), fmt))
        self._output_report(a, len(imgs), pieces, mode)

    def batch_palette_device(self, a):
        imgs = self._batch_images(a)
        k = a["k"]
        true = [self.ref.lloyd_triple(self.image_index(im), k) for im in imgs]
        results = self._chain(true, k)
        for j, (cent, it) in enumerate(results):
            a["cent"][j] = cent
            a["its"][j] = it
        its = [it for _, it in true]
        a["rep"][:] = (k + 2 + max(its), its[-1] if self.fault == "iterations_of_last_image" else max(its), 1, 0)

    def batch_apply_device(self, a):
        imgs = self._batch_images(a)
        mode, fmt, c4 = a["mode"], a["fmt"], a["c4"]
        t = self._batch_t()
        self._batch_refusals(a, t, False)
        if a["n_tables"] not in (1, len(imgs)):
            raise FakeError(-1, f"n_tables = {a['n_tables']}: 1 or n_images")
        self.scratch()
        for j, img in enumerate(imgs):
            cent = c4[0] if a["n_tables"] == 1 or self.fault == "per_image_tables_read_table_0" else c4[j]
            res = self._pass(img, cent, mode, fmt or None, t)
            self._put(a, j, res if fmt == 0 else self._indexed(res, fmt))
        self._output_report(a, len(imgs), [list(range(len(imgs)))], mode)

    def sequence(self):
        return FakeSequence(self)


class FakeSequence:
    """kmg_sequence_* with the library's kept state spelled out"""

    def __init__(self, proc):
        self.p, self.fault = proc, proc.fault
        self.block = None              # W: the compacted pixels of every frame, one array per frame
        self.cap = 0
        self.parts = []
        self.cutoffs = []
        self.frames = 0
        self.sw0 = self.sh0 = 0
        self.first_whole = False
        self.out = None
        self.last_record = None
        self.prev = None               # the centroids of the last local frame: they live in the sequence, not in the output
        self.wadd = 0                  # the weighting at the last add

    def close(self):
        self.end_output()
        if self.block is not None:
            self.p.give(self.block)
        self.block = None

    def _n(self):
        return sum(p.shape[0] for p in self.parts)

    def _add(self, img):
        p = self.p
        t = p.t if self.fault == "add_cutoff_ignores_weight" else p.wc()
        i = p.image_index(img)
        K, sw, sh, whole = p.ref.kept(i, t)
        self.wadd = p.w
        if self.fault == "cutoff_read_at_palette_time":
            K = p.ref.kept(i, 0)[0]                    # kept as it came: the compaction is left to the palette step
        need = 4 * (self._n() + sw * sh)
        if need > self.cap:                            # a new block of at least twice the size, the old one goes back
            new = p.take()
            if self.block is not None:
                p.give(self.block)
            if self.fault == "w_growth_drops_tail" and self.parts:
                self.parts[-1] = np.zeros_like(self.parts[-1])           # the copy stopped one frame short
            self.block, self.cap = new, max(need, 2 * self.cap)
        stale = self.fault == "clear_keeps_first_frame" and self.sw0 and not self.first_whole
        if self.frames == 0 and not stale:
            self.sw0, self.sh0, self.first_whole = sw, sh, whole
        self.parts.append(K)
        self.cutoffs.append(t)
        self.frames += 1

    def add(self, image):
        self._add(np.ascontiguousarray(image, np.uint8))

    def add_device(self, d_rgba, width, height, stream=0):
        self._add(_view(d_rgba, 4 * width * height, np.uint8).reshape(height, width, 4))

    def clear(self):
        self.parts, self.cutoffs, self.frames = [], [], 0
        if self.fault != "clear_keeps_first_frame":
            self.first_whole = False
            self.sw0 = self.sh0 = 0

    def info(self):
        return self.frames, self._n()

    def _centroids(self, k):
        p = self.p
        parts = self.parts
        if self.fault == "cutoff_read_at_palette_time":
            parts = [a[a[:, 3] >= p.t] if p.t else a for a in parts]
        n = sum(a.shape[0] for a in parts)
        if n == 0:
            raise FakeError(-1, "no pixel reaches alpha_cutoff")
        if k < p.n_fixed():
            raise FakeError(-1, "k is below the fixed colours")
        p.scratch()
        W = np.ascontiguousarray(np.concatenate(parts, axis=0))
        whole = self.first_whole if self.fault != "cutoff_read_at_palette_time" else n == self.sw0 * self.sh0
        as_image = self.frames == 1 and whole
        wt = self.wadd if self.fault == "weight_read_at_add" else p.w        # the weighting: as it is at the palette call
        return p.ref.centroids_px(W, self.sw0 if as_image else n, self.sh0 if as_image else 1, k, p.fid(), wt)

    def centroids(self, k):
        return self._centroids(k)

    def palette(self, k):
        return sorted_palette(self._centroids(k))

    def output(self, k, mode=0, format=1, width=0, height=0):
        self.end_output()
        if format != 0 and mode == 2:
            raise FakeError(-1, "meld has no index output")
        if format == 1 and k > 255:
            raise FakeError(-1, "INDEX8 holds 256 indices")
        cent = self._centroids(k)
        p = self.p
        block = p.take()
        canvas = np.full((height, width), k, np.int64)
        left = block.get("canvas")
        if self.fault == "canvas_survives_end_output" and left is not None and left.shape == canvas.shape:
            canvas = np.minimum(left, k)                                 # no fresh fill: what the block's last output showed
        self.out = dict(k=k, mode=mode, fmt=format, t=p.out_t(), cent=cent, canvas=canvas, held=np.zeros((height, width, 4), np.uint8),
                        frame=np.zeros((height, width, 4), np.uint8), block=block)
        self.last_record = None
        return p.ref.palette_bytes(cent)

    def end_output(self):
        if self.out is not None:
            for name in ("canvas", "shown", "held"):
                if name in self.out:
                    self.out["block"][name] = self.out[name]
            self.p.give(self.out["block"])
        self.out = None

    def output_local(self, k, mode=0, format=1, width=0, height=0, warm=False):
        self.end_output()                                                # a begin ends what was open before it checks its arguments
        if format not in (1, 2):
            raise FakeError(-1, "per-frame palettes need an index format")
        if mode == 2:
            raise FakeError(-1, "meld has no index output")
        if format == 1 and k > 255:
            raise FakeError(-1, "INDEX8 holds 256 indices")
        block = self.p.take()
        shown = np.zeros((height, width), np.uint32)                     # filled; the held source is not: what the block held
        left = block.get("shown")
        if self.fault == "shown_survives_begin" and left is not None and left.shape == shown.shape:
            shown = left.copy()
        held = block.get("held")
        if held is None or held.shape != (height, width, 4):
            held = np.full((height, width, 4), 0xCD, np.uint8)
        have_prev = self.fault == "warm_survives_begin" and self.prev is not None and self.prev.shape[0] == k
        self.out = dict(local=True, k=k, mode=mode, fmt=format, warm=bool(warm), t=self.p.t, shown=shown, held=held, have_prev=have_prev,
                        block=block)

    def frame_local(self, image, delta=True, tolerance=None):
        o = self.out
        if o is None or not o.get("local"):
            raise FakeError(-1, "no output with per-frame palettes is open")
        if tolerance is not None and not delta:
            raise FakeError(-1, "a lossy frame is a delta frame")
        p, k = self.p, o["k"]
        t = o["t"] if self.fault == "local_switches_read_at_begin" else p.t      # the switches: as they are when this call starts
        swapped = self.fault == "warm_after_failed_frame"                # which kind of failure forgets the last centroids
        if (o["warm"] and p.n_fixed()) or k < p.n_fixed():
            if swapped:
                o["have_prev"] = False
            raise FakeError(-5 if o["warm"] and p.n_fixed() else -1, "fixed colours")
        warm = o["warm"] and o["have_prev"]
        if not swapped:
            o["have_prev"] = False                                       # (the frame after one that failed in its palette step starts cold)
        img = np.ascontiguousarray(image, np.uint8)
        i = p.image_index(img)
        wt = 0 if self.fault == "warm_frame_unweighted" and warm else p.w    # the weighting, as the cutoff: read at this call
        tw = max(t, 1) if wt else t
        if p.ref.working(((i, tw),)) is None:
            if self.fault == "failed_frame_touches_shown":
                o["shown"] = np.zeros_like(o["shown"])
            raise FakeError(-1, "no pixel reaches alpha_cutoff")
        p.scratch()
        cent = p.ref.warm(i, tw, self.prev, wt) if warm else p.ref.centroids(((i, tw),), k, p.fid(), wt)
        if self.fault == "output_cutoff_follows_weight" and p.w and t == 0:
            t = 1
        I, P = p.ref.index(img, cent, o["mode"], t), p.ref.palette_bytes(cent)
        if tolerance is None:                                            # without delta the exact pass still runs: shown = P[I]
            d, o["shown"], rec = local_ref.colour(I, o["shown"], P, k)
            rec, full = tuple(rec) + (0, 0), (not delta) or rec[1] > 0
            if not delta:
                rec = local_ref.FRESH8
            o["held"] = img                                              # the frame buffer and the held source swap
        else:
            was_shown = o["shown"] != 0
            d, shown, held, rec = local_ref.lossy(O, img, I, o["shown"], o["held"], P, k, tolerance)
            if self.fault == "held_not_reanchored_local":
                held = np.where(was_shown[..., None], o["held"], held)
            full = rec[1] > 0
            if full:                                                     # the exact pass over the same canvas, and the swap
                if self.fault != "lossy_full_keeps_lossy_canvas":
                    shown = local_ref.lookup(I, P, k)[1]
                held = img
            o["shown"], o["held"] = shown, held
        self.prev, o["have_prev"] = cent, True
        return (I if full else d).astype(H.index_dtype(o["fmt"])), P, Record(rec), full

    def frame(self, image, delta=True, tolerance=None):
        o = self.out
        if o is not None and o.get("local"):
            raise FakeError(-1, "the open output has per-frame palettes")
        if o is None:
            raise FakeError(-1, "no output is open")
        if (delta or tolerance is not None) and o["fmt"] == 0:
            raise FakeError(-1, "a delta frame needs an index format")
        if tolerance is not None and not delta:
            raise FakeError(-1, "a lossy frame is a delta frame")
        p = self.p
        img = np.ascontiguousarray(image, np.uint8)
        t = p.t if self.fault == "plan_follows_cutoff" else o["t"]
        if o["fmt"] == 0:
            return p.ref.rgba(img, o["cent"], o["mode"], t), Record(sequence_ref.FRESH), True
        I = p.ref.index(img, o["cent"], o["mode"], t)
        k = o["k"]
        before = o["frame"]                                              # the frame buffer: what the last call uploaded
        o["frame"] = img
        if tolerance is None:
            d, o["canvas"], rec = sequence_ref.delta(I, o["canvas"], k)
            o["held"] = before if self.fault == "held_frame_swap_lost" else img   # the buffers swap: the held source is this frame
            full = (not delta) or rec[1] > 0
            if not delta:
                rec = sequence_ref.FRESH
            combine = sequence_ref.combine
        else:
            was_shown = o["canvas"] != k
            d, o["canvas"], held, rec = hold_ref.hold(O, img, I, o["canvas"], o["held"], k, tolerance)
            if self.fault == "held_not_reanchored":
                held = np.where(was_shown[..., None], o["held"], held)
            o["held"] = held
            full = rec[1] > 0
            if full:
                o["canvas"], o["held"] = I.copy(), (before if self.fault == "held_frame_swap_lost" else img)
            combine = hold_ref.combine
        if self.fault == "record_not_reset" and self.last_record is not None and len(self.last_record) == len(rec) and delta:
            rec = combine(self.last_record, rec)
        self.last_record = tuple(rec)
        return (I if full else d).astype(H.index_dtype(o["fmt"])), Record(rec), full


class FakeLloyd:
    """the part of kmg_lloyd_* the session harness drives: per-pixel passes over whole images, n_fixed with the object"""

    def __init__(self, proc, k, fault=None):
        self.p, self.k, self.fault = proc, int(k), fault
        self.cent = np.zeros((self.k, 4), np.float32)
        self.nconv = 0
        self.block = proc.take()
        self.f = min(self.block.get("n_fixed", 0), self.k) if fault == "n_fixed_inherited" else 0   # the device word of the block's last owner
        self.bound = None              # the caller's binding
        self.init_bound = None         # the binding the initialisation left (forced colour table)
        self.w = self.block.get("weighted", 0) if fault == "lloyd_weight_inherited" else 0
        self.plain = None              # the pixel counts of the last weighted pass

    def close(self):
        self.block["n_fixed"] = self.f
        self.block["weighted"] = self.w
        self.p.give(self.block)

    def set_weighting(self, v):
        if v not in (0, 1):
            raise FakeError(-1, "unknown weighting")
        if self.bound is not None and self.fault != "weight_set_under_binding":
            raise FakeError(-1, "an image is bound")
        if v != self.w and self.fault != "weighted_object_uses_binding":
            self.init_bound = None                                       # ends in both directions
        self.w = int(v)

    def _wt(self, d_rgba, n):
        """are the sums of a pass over these pixels weighted?"""
        if self.fault == "weighted_object_uses_binding" and self.init_bound == (d_rgba, n):
            return 0
        return self.w

    def _image(self, ptr, n):
        return self.p.image_index(_view(ptr, 4 * n, np.uint8))

    def _step(self, sums):
        self.cent, self.nconv = fixed_ref.step(O, np.ascontiguousarray(sums), self.cent, self.f)

    def _acc(self, d_acc):
        return _view(d_acc, 4 * self.k, np.int64).reshape(self.k, 4)

    def set_centroids(self, c, stream=0):
        self.cent = np.ascontiguousarray(c, np.float32).reshape(self.k, 4).copy()

    def get_centroids(self, stream=0):
        out = self.cent.copy()
        out[:, 3] = 1.0
        return out

    def init_centroids_seeded(self, d_rgba, w, h, seeds4, stream=0):
        f = np.asarray(seeds4).reshape(-1, 4).shape[0]
        if f > self.k:
            raise FakeError(-1, "more seeds than centroids")
        self.cent = self.p.ref.seeded(self._image(d_rgba, w * h), self.k, f)
        if self.p.strategy == 2 and self.k > 1:                          # over the colour table: the image stays bound, by the library
            self.init_bound, self.bound = (d_rgba, w * h), None

    def set_fixed(self, n_fixed):
        if n_fixed > self.k:
            raise FakeError(-1, "n_fixed > k")
        if n_fixed == 0 and self.fault == "set_fixed_zero_ignored":
            return
        self.f = int(n_fixed)

    def bind_image(self, d_rgba, n, stream=0):
        if self.w:
            raise FakeError(-1, "the object's sums are weighted")
        self.bound, self.init_bound = (d_rgba, n), None

    def unbind_image(self):
        self.bound = self.init_bound = None

    def converged_count(self, stream=0):
        return self.nconv

    def update(self, d_acc, stream=0):
        sums = self._acc(d_acc).copy()
        if self.fault == "zero_weight_cluster_counts_pixels" and self.w and self.plain is not None and self.plain.shape == sums.shape:
            rows = (sums[:, 3] == 0) & (self.plain[:, 3] > 0)            # "not empty": it has pixels
            sums[rows] = self.plain[rows]
        self._step(sums)

    def assign_accumulate(self, d_rgba, n, d_labels, d_acc, stream=0):
        i, wt = self._image(d_rgba, n), self._wt(d_rgba, n)
        labels, sums = self.p.ref.assign(i, self.cent, wt)
        self.plain = self.p.ref.assign(i, self.cent, 0)[1] if wt else None
        if d_labels:
            _view(d_labels, n, np.uint32)[:] = labels
        if d_acc:
            self._acc(d_acc)[:] = sums

    def assign_update(self, d_rgba, n, d_labels, d_acc, do_update=True, stream=0):
        self.assign_accumulate(d_rgba, n, d_labels, d_acc)
        if do_update:
            self.update(d_acc)

    def iterate(self, d_rgba, n, d_labels, d_acc, update_first=True, stream=0):
        if update_first:
            self.update(d_acc)
        self.assign_accumulate(d_rgba, n, d_labels, d_acc)

    def flush(self, stream=0):
        pass

    def run(self, d_rgba, n, d_labels=0, stream=0):
        self.cent, labels, it = self.p.ref.run(self._image(d_rgba, n), self.cent, self.f, self._wt(d_rgba, n))
        self.init_bound = None                                           # made or taken over for this run, dropped before it returns
        self.nconv = 0
        if d_labels:
            _view(d_labels, n, np.uint32)[:] = labels
        return it

    def accumulate_into(self, d_rgba, n, d_acc, stream=0):
        if self.w:
            raise FakeError(-1, "the object's sums are weighted")
        if self.bound != (d_rgba, n):
            raise FakeError(-1, "the image is not bound")
        self._acc(d_acc)[:] += self.p.ref.assign(self._image(d_rgba, n), self.cent)[1]

    def labels_from_tables_update(self, d_rgba, n, d_labels, d_acc, stream=0):
        if self.w:
            raise FakeError(-1, "the object's sums are weighted")
        if self.bound is None:
            raise FakeError(-1, "no bound image")
        if self.k > 256:
            raise FakeError(-5, "k <= 256")
        _view(d_labels, n, np.uint32)[:] = self.p.ref.assign(self._image(d_rgba, n), self.cent)[0]
        acc = self._acc(d_acc)
        self._step(acc.copy())
        acc[:] = 0


class FakeEnv:
    Error = FakeError

    def __init__(self, images, cache, fault=None):
        self.fault, self.images, self.cache = fault, images, cache
        self.mem = HostMem()
        self.streams = [0, 0]

    def sync(self):
        pass

    def session_processor(self):
        return FakeProcessor(self.fault, self.images, self.cache)

    def lloyd(self, proc, k):
        return FakeLloyd(proc, k, self.fault)

    def set_weighting(self, proc, value):
        proc.set_weighting(value)

    def index_plan(self, usage, palette, flags):
        planned = index_ref.plan(usage, palette, flags)
        if planned is None:
            raise FakeError(-1, "the plan refuses")
        return planned

    def batch(self, proc, a):
        try:
            getattr(proc, "batch_" + a["call"][2:])(a)
        except FakeError as e:
            return e.status, str(e)
        return 0, ""

    def fresh_hold(self):
        return np.array(hold_ref.FRESH[:2], np.uint64).tobytes() + np.array(hold_ref.FRESH[2:6], np.uint32).tobytes() + \
            np.array(hold_ref.FRESH[6:], np.uint64).tobytes()


def _env(seed, seq, cache, fault=None):
    return FakeEnv(H.make_images(seed, seq), cache, fault)


def _campaign(seeds, faults, surface):
    """every committed (seed, sequence) on the faithful stand-in and on each faulty one that seed has not caught yet"""
    O.lib()
    counters = collections.Counter()
    caught = {seed: {} for seed in seeds}
    failures, reused, n_ops = [], {}, 0
    for seed in seeds:
        reused[seed] = []
        for seq in range(SEQUENCES):
            answers = {}                          # the reference's answers: the same for every stand-in of this sequence
            ops = H.generate(seed, seq, surface=surface)
            try:
                done, _, again = H.run_sequence(_env(seed, seq, answers), seed, seq, ops, counters, cache=answers)
                reused[seed].append(again)
                n_ops += done
            except H.Mismatch as e:
                failures.append(str(e)[:3000])
            for fault in faults:
                if fault in caught[seed]:
                    continue
                try:
                    H.run_sequence(_env(seed, seq, answers, fault), seed, seq, ops, cache=answers)
                except H.Mismatch as e:
                    caught[seed][fault] = (seq, str(e).split("\n")[0][:200])
    return {"counters": counters, "caught": caught, "failures": failures, "reused": reused, "ops": n_ops}


@pytest.fixture(scope="module")
def campaign():
    return _campaign(SEEDS, FAULTS, 1)


@pytest.fixture(scope="module")
def campaign_2():
    return _campaign(SEEDS_2, FAULTS + FAULTS_2, 2)


@pytest.fixture(scope="module")
def campaign_3():
    return _campaign(SEEDS_3, FAULTS + FAULTS_2 + FAULTS_3, 3)


@pytest.fixture(scope="module")
def campaign_4():
    return _campaign(SEEDS_4, FAULTS_4, 4)


def test_generator_is_deterministic():
    assert H.generate(SEEDS[0], 1) == H.generate(SEEDS[0], 1)
    assert H.generate(SEEDS[0], 1) != H.generate(SEEDS[1], 1)
    ops = H.generate(SEEDS[0], 0)
    assert eval(repr(ops)) == ops                      # a sequence is a list of plain tuples: the printed list replays
    a, b = H.make_images(SEEDS[0], 1), H._make_images(SEEDS[0], 1)
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_faithful_stand_in_passes_every_sequence(campaign):
    assert not campaign["failures"], "\n\n".join(campaign["failures"])
    assert all(n > 0 for seed in SEEDS for n in campaign["reused"][seed]) and all(len(campaign["reused"][s]) == SEQUENCES for s in SEEDS), \
        campaign["reused"]


def test_faithful_stand_in_passes_every_sequence_of_surface_2(campaign_2):
    assert not campaign_2["failures"], "\n\n".join(campaign_2["failures"])
    reused = campaign_2["reused"]
    assert all(n > 0 for seed in SEEDS_2 for n in reused[seed]) and all(len(reused[s]) == SEQUENCES for s in SEEDS_2), reused


def test_faithful_stand_in_passes_every_sequence_of_surface_3(campaign_3):
    assert not campaign_3["failures"], "\n\n".join(campaign_3["failures"])
    reused = campaign_3["reused"]
    assert all(n > 0 for seed in SEEDS_3 for n in reused[seed]) and all(len(reused[s]) == SEQUENCES for s in SEEDS_3), reused


def test_faithful_stand_in_passes_every_sequence_of_surface_4(campaign_4):
    assert not campaign_4["failures"], "\n\n".join(campaign_4["failures"])
    reused = campaign_4["reused"]
    assert all(n > 0 for seed in SEEDS_4 for n in reused[seed]) and all(len(reused[s]) == SEQUENCES for s in SEEDS_4), reused


# sha256 of repr(generate(seed, seq)) on the commit before surface 2 existed: the sessions of the old seeds never change
PINNED = {
    201: ("9583056de68e9607bd6dc48e57fac0e98ea9ef1e700e99f80ff67861f48a5309", "a9220eb11068dd3887b9e29b693f33ad6198d868f915388d85772889113eec54",
          "e258aeb19305343aed8cdf3b7ca1f860acf23702a782312c43c4233bfdf9ea9b", "54b695d69c1eb3d23db5c8db72bb3c9b45ae19d97435c6f2dfe9fd541a3e4470",
          "b87c37e3a40f5d685370ab682c6eea800065861e14c76396875ea2f456c72bd1", "4c0a60228005c39d972e225bbc420b10ef493a101460781c7e77b47644a64b78"),
    202: ("656bc1cc05998d6ddb2399629ad7e7f02a49db17fc31df209875cab3a7df1207", "7ef1e222f1dc1559c410fa6e9b4f24f962b3ce6db7cd112d5d51d0bebea006cb",
          "dbf61297a835f5e39a63bc7e2bad3825078a126864306ab9d4a0e069362965c2", "b39ddf06b2c417efa46d86c40bfbefbcb610e29e724ef21da68d1356ae84dbe2",
          "3035460b8c40bd9e7d23d242ccead673b1132903efde7f233640f793cbfc5975", "f8737bebd5eb4efddea290d3d1cac4ddb4b02a765c588e693adedb78adc352b0"),
}


# ... and of repr(generate(seed, seq, surface=2)) on the commit before surface 3 existed
PINNED_2 = {
    314: ("49309b4d407ca09b47f663d4c30ed2b2b0c5a53e1fec61e22009f921cfd97609", "201513196dab6bb60bfc7e09fa09350b16a174619006d6be3fae7dca730190c7",
          "55d9f5daff0eaeb6e48cb0580a2498033d3aa4fa2641a2898141851a757c6695", "76c916704ac61e08ad3de1bb040da159f5e57e2d202c92bf0589cbe5cfef71ae",
          "88aa550a65ed86108bdc714bc8108dcb447991a2c9b419a245d46b122f3911e0", "ccdd01752634f5d2dc2a45280daaf73d2eb028050e469a65d51905d3bf395ee5"),
    315: ("6e11c95f09439fdc1f5f528b02f38ce7b040f2373a6d9a0d83ab9269f04ebcef", "0b8ec27d1b6ff7e3bd7b7ef8735d4c8eaa15ebecd93526ed04d6cc340249f7c5",
          "9765e08acd84064eb4f7d38b1d92fe5edeba024442b3deaac34b3d7c191198a6", "fcd694726c11c0c0ffa60c474b7bc7a11a6799ee6e35ee7d695db959344443d8",
          "8699f6627162b8a739234f6d14431033426a04862b568d272d4f826ba1d1fd24", "0a951a1aac38858d12d3c6dad528548e0cdd9a929358253aa53c80a920b41331"),
}
# ... of repr(generate(seed, seq, surface=3)) on the commit before surface 4 existed
PINNED_3 = {
    421: ("ea72033d6d80006f4d9029e3dea242728a8c739d462be243c0c9c8c39faf417b", "dd00d5cf53402dfbb3c15bfe3e4fff4d4dc21ffd9c739677c61b26ba20908fbc",
          "bdfc865d99626729996bb4993db34ef18c603355ca9d8b0e1d8c69291f840273", "d41facc2e879d7b809ad5128cd4b04f46d9ca9a382aaf567d66d2ec0da6252ef",
          "a928e98364454e1190fc00bb4b5f819b8763e5306011c50ee7e14bd9dc366a5d", "066921f160d7e9ef055799076c5b07902b609d2f116bb46197a0d3441e1913a6"),
    422: ("9c0d84e0d648d5617cf1629380e172c7db4dfd10e1a6db78af84159febbbeade", "6393f1ac88529fed21e2163ed9233777f7102d59675142dc8d2849157a27f02c",
          "6196c5b3c953cb2dc79f5f6e6dade51eb91268f38c4b1c4cb52f369d3a5c3c03", "a840107b70aff802cd20d67f7f88b0efcca0ef754b01f2e89d037dc8a86538cd",
          "5530ca1e74ea34dd71566a7e165c9f39a754e80b3d0a4f8fc6c686d15e075bfd", "b9e704f483873327f7d303e483181ac38f7e8a1ddbe64507d59419fe327bdfb3"),
}
# ... and of repr(generate(seed, seq, surface=4)): the sessions tests/test_gpu_session.py runs and the counts of EXACT_4
PINNED_4 = {
    533: ("ad497ddd08dbc0a50e987338cf21904db926f718a0d0088798c0cfe53830f505", "8351a62d49201a4c566c3d49d0ea8776389653bd2af294f56c7dcc9c7874e6aa",
          "fca5d5ee0ac741a48d54b8f44180d3625585754d55db345e1895e7434cbd70b7", "876020a91bd90588af4e7d68c47e43e5733a46819c73a4371fa74a27f4d885cf",
          "92fd0e42c68f4c93ad387b6e5d25b19c52df1576f5ad0652c31eb3cbae295729", "14525f7e8b1b8a4f9f370364fd374939b779398534e0a897b424f81e77525c6b"),
    534: ("d541c3ad00b085730dd3e8d33a0f06bad3c7d5fedc63799d8edd8803089ed999", "b2c7dd932a2a97bf31fc3e09e38d40acf352b61c5e60697b38f0225033f0f440",
          "32751133cb3a7dc3fa9e00d5e5d66dc5750063a8e96ff5145fdf26c1cab0bf29", "1ed0f78b32c4a31ca27c894306f74e4a8bbd9362950f9a8756390f2612f2c0a2",
          "ac3f70a7c2ed089af65589eed00e16fa061d2c0890f96e166976c52d0c556a9a", "0abbd29da2924a72cca7f5cbf15d69546cd954099720acf7277fd9aef29bc047"),
}
# sha256 over the bytes of the fourteen images of make_images(seed, 0) that existed before the importance map was appended
PINNED_IMAGES = {201: "851b8715dfdba15b", 314: "791765901562b45a", 7: "cfdc31856e48d6fc"}


@pytest.mark.parametrize("seed", SEEDS_2)
def test_the_committed_sessions_of_surface_2_are_as_they_were(seed):
    assert len(PINNED_2[seed]) == SEQUENCES
    for seq in range(SEQUENCES):
        ops = H.generate(seed, seq, surface=2)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == PINNED_2[seed][seq], (seed, seq)
        assert ops != H.generate(seed, seq, surface=3)
        assert not {op[0] for op in ops} & set(NEW_OPS_3) and not {op[1] for op in ops if op[0] == "refuse"} & set(H.REFUSALS_3)
        assert not any(op[1] == H.MAP for op in ops if op[0] in ("palette", "reduce", "reduce_indexed", "quality")) and \
            not any(op[2] == H.MAP for op in ops if op[0] == "s_add")


@pytest.mark.parametrize("seed", SEEDS_3)
def test_the_committed_sessions_of_surface_3_are_as_they_were(seed):
    assert len(PINNED_3[seed]) == SEQUENCES
    for seq in range(SEQUENCES):
        ops = H.generate(seed, seq, surface=3)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == PINNED_3[seed][seq], (seed, seq)
        assert ops != H.generate(seed, seq, surface=4)
        assert not {op[0] for op in ops} & set(NEW_OPS_4) and not {op[1] for op in ops if op[0] == "refuse"} & set(H.REFUSALS_4)
        assert not {op[1] for op in ops if op[0] == "motif"} & set(H.MOTIFS_4)


@pytest.mark.parametrize("seed", SEEDS_4)
def test_the_committed_sessions_of_surface_4_are_pinned(seed):
    assert len(PINNED_4[seed]) == SEQUENCES
    for seq in range(SEQUENCES):
        ops = H.generate(seed, seq, surface=4)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == PINNED_4[seed][seq], (seed, seq)
        assert eval(repr(ops)) == ops


@pytest.mark.parametrize("seed", sorted(PINNED_IMAGES))
def test_the_images_are_as_they_were(seed):
    images = H.make_images(seed, 0)
    assert [k for k, _ in images] == list(H.IMAGE_KINDS) and H.IMAGE_KINDS[H.MAP] == "map"
    assert hashlib.sha256(b"".join(a.tobytes() for _, a in images[:14])).hexdigest()[:16] == PINNED_IMAGES[seed]
    wmap = images[H.MAP][1]
    assert wmap.shape == (67, 53, 4) and wmap[..., 3].min() >= 1            # every pixel kept at t <= 1: the working image is 2-D


@pytest.mark.parametrize("seed", SEEDS)
def test_the_committed_sessions_are_as_they_were(seed):
    assert len(PINNED[seed]) == SEQUENCES
    for seq in range(SEQUENCES):
        ops = H.generate(seed, seq)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == PINNED[seed][seq], (seed, seq)
        assert ops == H.generate(seed, seq, surface=1) and ops != H.generate(seed, seq, surface=2)
        assert not {op[0] for op in ops} & set(NEW_OPS) and not {op[1] for op in ops if op[0] == "refuse"} & set(H.REFUSALS_2)


@pytest.mark.parametrize("fault", FAULTS)
def test_every_seed_catches_the_faulty_stand_in(campaign, fault):
    for seed in SEEDS:
        assert fault in campaign["caught"][seed], f"seed {seed} does not catch {fault} in {SEQUENCES} sequences"


@pytest.mark.parametrize("fault", FAULTS + FAULTS_2)
def test_every_seed_of_surface_2_catches_the_faulty_stand_in(campaign_2, fault):
    for seed in SEEDS_2:
        assert fault in campaign_2["caught"][seed], f"seed {seed} does not catch {fault} in {SEQUENCES} sequences"


@pytest.mark.parametrize("fault", FAULTS + FAULTS_2 + FAULTS_3)
def test_every_seed_of_surface_3_catches_the_faulty_stand_in(campaign_3, fault):
    for seed in SEEDS_3:
        assert fault in campaign_3["caught"][seed], f"seed {seed} does not catch {fault} in {SEQUENCES} sequences"


@pytest.mark.parametrize("fault", FAULTS_4)
def test_every_seed_of_surface_4_catches_the_faulty_stand_in(campaign_4, fault):
    for seed in SEEDS_4:
        assert fault in campaign_4["caught"][seed], f"seed {seed} does not catch {fault} in {SEQUENCES} sequences"


def _replays(caught, seed, fault, surface):
    """the replay(...) line a failing run prints runs again: it fails on the faulty stand-in and passes on the faithful one"""
    seq, _ = caught[seed][fault]
    with pytest.raises(H.Mismatch) as e:
        H.run_sequence(_env(seed, seq, {}, fault), seed, seq, surface=surface)
    text = str(e.value)
    assert f"seed {seed} sequence {seq}: op " in text
    ops = eval(text[text.index("replay(env, "):].split(", ", 3)[3][:-1])
    with pytest.raises(H.Mismatch):
        H.replay(_env(seed, seq, {}, fault), seed, seq, ops)
    assert H.replay(_env(seed, seq, {}), seed, seq, ops)[0] == len(ops)
    return ops


def test_a_mismatch_prints_a_list_that_replays(campaign, campaign_2, campaign_3, campaign_4):
    _replays(campaign["caught"], SEEDS[0], "plan_follows_cutoff", 1)
    ops = _replays(campaign_2["caught"], SEEDS_2[0], "lossy_full_keeps_lossy_canvas", 2)        # a printed list of surface 2
    assert {op[0] for op in ops} & set(NEW_OPS)
    ops = _replays(campaign_3["caught"], SEEDS_3[0], "weight_read_at_add", 3)                   # ... and of surface 3
    assert {op[0] for op in ops} & set(NEW_OPS_3)
    ops = _replays(campaign_4["caught"], SEEDS_4[0], "stale_stop_word", 4)                      # ... and of surface 4
    assert {op[0] for op in ops} & set(NEW_OPS_4)
    ops = _replays(campaign_4["caught"], SEEDS_4[1], "refused_batch_writes_first_sub_batch", 4)
    assert ops[-1][:2] == ("refuse", "batch_no_kept_pixel")


@pytest.mark.parametrize("seed", SEEDS)
def test_vectorised_references_equal_their_loop_forms(seed):
    """the model uses hold_ref.hold and the anti-diagonal diffusion; once per seed they are held against the literal per-pixel
    loops (hold_ref.hold_loop, alpha_ref.diffuse_serial), and the index diffusion against the RGBA8 one"""
    images = H.make_images(seed, 0)
    rng = np.random.default_rng(seed)
    for t in (0, 128):
        img = np.ascontiguousarray(images[H.COL][1] if t else images[H.ROW][1])
        crop = np.ascontiguousarray(images[H.SPRITE][1][20:44, 30:60])
        cent, _ = H.gamut_centroids(seed, 9)
        P = O.lab_to_rgba8(cent[:, :3])
        for a in (img, crop):
            idx = H.diffuse_index(a, cent, t)
            want = alpha_ref.diffuse_serial(a, diffuse_ref.oracle_apply_replace(O, cent), t)
            assert np.array_equal(P[idx][..., :3], want[..., :3])
            assert np.array_equal(alpha_ref.diffuse(a, diffuse_ref.oracle_apply_replace(O, cent), t), want)
    src, nxt = images[H.SPRITE][1][10:40, 20:60], images[3][1][10:40, 20:60]
    index = rng.integers(0, 6, src.shape[:2])
    canvas = np.where(rng.random(src.shape[:2]) < 0.3, 5, rng.integers(0, 6, src.shape[:2]))
    for tol in (0, 40, 4096):
        got = hold_ref.hold(O, nxt, index, canvas, src, 5, tol, row0=3)
        want = hold_ref.hold_loop(O, nxt, index, canvas, src, 5, tol, row0=3)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and tuple(got[3]) == tuple(want[3])


def _scenarios():
    import test_gpu_session as G
    return G


@pytest.mark.parametrize("name", ["cutoff_0_128_0_around_palette_reduce_and_a_plan", "frames_added_under_three_cutoffs_then_clear",
                                  "an_output_ends_a_lloyd_object_runs_in_its_block_and_the_next_output_starts_fresh",
                                  "frozen_seeds_do_not_outlive_their_object", "quality_search_with_and_without_pins_beside_a_bound_object",
                                  "records_combine_over_bands_in_reverse_on_two_streams", "every_refusal_is_followed_by_the_correct_call",
                                  "two_sequences_alternate_beside_host_calls_on_the_megapixel_image",
                                  "a_warm_output_across_a_cutoff_switch_and_back",
                                  "a_refused_frame_leaves_a_warm_output_warm_and_a_failed_palette_step_makes_it_cold",
                                  "a_local_output_begins_in_a_used_block_with_a_lossy_first_frame",
                                  "a_lossy_frame_comes_back_in_full_then_an_exact_and_a_lossy_frame",
                                  "local_shared_local_on_one_sequence_with_the_refusals_between",
                                  "the_sequence_optimize_path_counts_plans_remaps_and_replays",
                                  "usage_records_outlive_their_maps_and_the_bad_count_combines",
                                  "a_colour_keyed_canvas_of_the_caller_on_both_routes",
                                  "weight_on_cutoff_0_128_0_weight_off_around_the_same_calls",
                                  "two_frames_added_under_different_weightings_and_the_palette_both_ways",
                                  "a_warm_output_alternates_weighted_and_unweighted_frames_across_a_cutoff_switch",
                                  "the_binding_of_an_initialisation_and_of_the_caller_around_the_lloyd_weighting",
                                  "weighted_and_unweighted_lloyd_objects_in_each_others_blocks_beside_weighted_host_calls",
                                  "fixed_colours_and_weighting_with_clusters_of_weight_0",
                                  "the_quality_search_weighted_then_unweighted",
                                  "batches_of_nine_two_and_one_image_at_k_300_3_and_33",
                                  "two_device_batches_with_a_lloyd_object_in_the_block_between",
                                  "cutoff_0_128_0_around_the_indexed_and_the_find_batch_then_device_output_batches",
                                  "fixed_colours_and_weighting_around_the_batches",
                                  "a_batch_refused_for_an_image_without_a_kept_pixel_then_the_same_list_without_it",
                                  "batches_between_the_frames_of_an_open_output_and_beside_a_bound_lloyd_object",
                                  "octree_batches_alternate_with_k_means_batches"])
def test_the_named_scenarios_of_the_device_are_legal_sequences(name):
    """the op lists tests/test_gpu_session.py runs on the device, on the faithful stand-in (one processor per list here)"""
    G = _scenarios()
    assert set(G.SCENARIOS) >= {name}
    ops = G.SCENARIOS[name]()
    answers = {}
    assert H.run_sequence(_env(G.SEED, G.SEQ, answers), G.SEED, G.SEQ, ops, cache=answers)[0] == len(ops)


def test_every_scenario_of_the_device_is_checked_here():
    G = _scenarios()
    names = test_the_named_scenarios_of_the_device_are_legal_sequences.pytestmark[0].args[1]
    assert sorted(G.SCENARIOS) == sorted(names)


# what the committed seeds give (SEEDS x SEQUENCES), exactly: the generator is deterministic.  None may be zero.
EXACT = {
    'op:cutoff': 82, 'op:fixed': 68, 'op:strategy': 25, 'op:palette': 62, 'op:reduce': 26, 'op:reduce_indexed': 32, 'op:find':
    12, 'op:find_indexed': 22, 'op:quality': 47, 'op:apply': 80, 'op:apply_plan': 38, 'op:compact': 16, 'op:compare_device': 36,
    'op:pair_open': 24, 'op:pair_frame': 108, 'op:l_new': 29, 'op:l_re': 38, 'op:l_close': 29, 'op:l_set': 37, 'op:l_init': 30,
    'op:l_fix': 52, 'op:l_bind': 4, 'op:l_conv': 21, 'op:l_update': 18, 'op:l_assign': 11, 'op:l_assign_update': 48,
    'op:l_iterate': 10, 'op:l_run': 15, 'op:l_lftu': 13, 'op:s_new': 31, 'op:s_close': 31, 'op:s_add': 178, 'op:s_clear': 75,
    'op:s_info': 39, 'op:s_centroids': 32, 'op:s_palette': 15, 'op:s_output': 98, 'op:s_end': 18, 'op:s_frame': 245,
    'op:refuse': 67, 'refusal:k_below_fixed_palette': 8, 'refusal:k_below_fixed_reduce': 7, 'refusal:k_below_fixed_sequence': 1,
    'refusal:octree_fixed': 9, 'refusal:frame_no_output': 5, 'refusal:delta_on_rgba8': 4, 'refusal:lossy_on_rgba8': 8,
    'refusal:lossy_without_delta': 8, 'refusal:index8_full': 4, 'refusal:meld_indexed': 10, 'refusal:empty_sequence': 3,
    'k:0:rgba8': 20, 'k:0:index8': 22, 'k:0:index16': 10, 'k:1:rgba8': 112, 'k:1:index8': 91, 'k:1:index16': 52, 'k:2:rgba8':
    21, 'k:2:index8': 42, 'k:2:index16': 17, 'k:3:rgba8': 11, 'k:3:index8': 3, 'k:3:index16': 3, 'k:4:rgba8': 2, 'k:4:index16':
    12, 'transition:exact>lossy': 46, 'transition:lossy>exact': 30, 'is_full_fallback': 46, 'frame_held_pixels': 21,
    'mixed_cutoff_sequence': 28, 'plan_outlives_cutoff': 38, 'reoutput': 53, 'add_shrunk': 8, 'compare_host': 20,
    'record_combined_across_images': 14, 'set_fixed_zero': 10, 'set_fixed': 42, 'pair_exact': 20, 'pair_lossy': 88,
    'frame_exact': 159, 'frame_lossy': 86, 'update_with_n_fixed:l_update': 9, 'update_with_n_fixed:l_assign_update': 10,
    'update_with_n_fixed:l_iterate': 5, 'update_with_n_fixed:l_run': 6, 'update_with_n_fixed:l_lftu': 6, 'compare_bands:1': 21,
    'compare_bands:2': 9, 'compare_bands:3': 6, 'delta_bands:1': 50, 'delta_bands:2': 29, 'delta_bands:3': 29, 'fixed:0': 26,
    'fixed:1': 3, 'fixed:2': 17, 'fixed:3': 22,
}


def coverage_names():
    formats = {0: ("rgba8", "index8", "index16"), 1: ("rgba8", "index8", "index16"), 2: ("rgba8", "index8", "index16"),
               3: ("rgba8", "index8", "index16"), 4: ("rgba8", "index16")}
    return ["op:" + o for o in ("cutoff", "fixed", "strategy", "palette", "reduce", "reduce_indexed", "find", "find_indexed", "quality", "apply",
                                "apply_plan", "compact", "compare_device", "pair_open", "pair_frame", "l_new", "l_re", "l_close", "l_set", "l_init",
                                "l_fix", "l_bind", "l_conv", "l_update", "l_assign", "l_assign_update", "l_iterate", "l_run", "l_lftu", "s_new",
                                "s_close", "s_add", "s_clear", "s_info", "s_centroids", "s_palette", "s_output", "s_end", "s_frame", "refuse")] + \
           ["refusal:" + r for r in H.REFUSALS_1] + [f"k:{cls}:{f}" for cls, fs in formats.items() for f in fs] + \
           ["transition:exact>lossy", "transition:lossy>exact", "is_full_fallback", "frame_held_pixels", "mixed_cutoff_sequence",
            "plan_outlives_cutoff", "reoutput", "add_shrunk", "compare_host", "record_combined_across_images", "set_fixed_zero", "set_fixed",
            "pair_exact", "pair_lossy", "frame_exact", "frame_lossy"] + \
           ["update_with_n_fixed:" + n for n in ("l_update", "l_assign_update", "l_iterate", "l_run", "l_lftu")] + \
           [f"compare_bands:{n}" for n in (1, 2, 3)] + [f"delta_bands:{n}" for n in (1, 2, 3)] + [f"fixed:{i}" for i in range(4)]


def test_coverage_of_the_committed_seeds(campaign):
    c = campaign["counters"]
    print(dict(sorted(c.items())), campaign["ops"])
    assert not campaign["failures"]
    need = coverage_names()
    assert set(need) == set(EXACT), sorted(set(need) ^ set(EXACT))
    wrong = {name: (c[name], EXACT[name]) for name in need if c[name] != EXACT[name] or EXACT[name] < 1}
    assert not wrong, wrong
    assert all(n > 0 for seed in SEEDS for n in campaign["reused"][seed])          # blocks re-used, in every sequence


# what the committed seeds of surface 2 give (SEEDS_2 x SEQUENCES), exactly, for what surface 2 adds.  None may be zero.
EXACT_2 = {
    'op:s_output_local': 117, 'op:s_frame_local': 328, 'op:cpair_open': 26, 'op:cpair_frame': 93, 'op:usage_device': 46,
    'op:plan': 29, 'op:remap_device': 40, 'op:optimize': 25, 'op:s_usage': 32, 'op:s_remap': 29,
    'refusal:shared_frame_on_local': 12, 'refusal:local_frame_on_shared': 14, 'refusal:local_frame_no_output': 3,
    'refusal:warm_with_fixed': 2, 'refusal:local_tolerance_without_delta': 4, 'refusal:local_meld': 2,
    'refusal:local_index8_k256': 1, 'refusal:plan_indices_above_k': 4, 'refusal:plan_empty_record': 3,
    'refusal:optimize_bits_too_narrow': 2, 'refusal:remap_bad_bits': 3, 'local_warm': 108, 'local_cold': 190, 'local_exact':
    175, 'local_lossy': 123, 'local_begin_warm': 70, 'local_begin_cold': 47, 'local_first_frame_lossy': 29, 'local_lossy_full':
    41, 'local_held_pixels': 64, 'local_cutoff_differs_from_last_frame': 16, 'failed_frame:fixed_on_warm': 12,
    'failed_frame:k_below_fixed': 10, 'failed_frame:empty': 10, 'frame_after_failed:fixed_on_warm': 12,
    'frame_after_failed:k_below_fixed': 10, 'frame_after_failed:empty': 10, 'cpair_exact': 39, 'cpair_lossy': 54,
    'route:vector': 51, 'route:per_pixel': 42, 'cdelta_bands:1': 49, 'cdelta_bands:2': 10, 'cdelta_bands:3': 34, 'remap_bits:1':
    11, 'remap_bits:2': 12, 'remap_bits:4': 2, 'remap_bits:8': 36, 'remap_bits:16': 8, 'plan_order:0': 6, 'plan_order:1': 14,
    'plan_order:2': 9, 'plan_flag:4': 8, 'plan_flag:8': 14, 'plan_flag:16': 7, 'usage:index8:0': 6, 'usage:index8:1': 4,
    'usage:index8:2': 5, 'usage:index8:3': 12, 'usage:index16:0': 3, 'usage:index16:1': 10, 'usage:index16:2': 3,
    'usage:index16:3': 1, 'usage:index16:4': 2, 'usage_fresh': 34, 'usage_combined_across_images': 12, 'usage_bands:1': 6,
    'usage_bands:2': 22, 'usage_bands:3': 18, 's_usage_fresh': 14, 's_usage_combined': 18, 'remap_in_place': 7,
    'remap_planned_table': 14, 'remap_random_table': 26, 'bad_count_combined': 18, 'optimize_plan_bits': 8,
    'optimize_given_bits': 17, 'optimize_path_replayed': 9,
}


def coverage_names_2():
    """what surface 2 adds (the old names are EXACT's and are counted there on the old seeds)"""
    return ["op:" + o for o in NEW_OPS] + ["refusal:" + r for r in H.REFUSALS_2] + \
           ["local_warm", "local_cold", "local_exact", "local_lossy", "local_begin_warm", "local_begin_cold", "local_first_frame_lossy",
            "local_lossy_full", "local_held_pixels", "local_cutoff_differs_from_last_frame"] + \
           ["failed_frame:" + k for k in H.FAILED_KINDS] + ["frame_after_failed:" + k for k in H.FAILED_KINDS] + \
           ["cpair_exact", "cpair_lossy", "route:vector", "route:per_pixel"] + [f"cdelta_bands:{n}" for n in (1, 2, 3)] + \
           [f"remap_bits:{b}" for b in H.BITS] + [f"plan_order:{o}" for o in (0, 1, 2)] + [f"plan_flag:{b}" for b in (4, 8, 16)] + \
           [f"usage:index8:{c}" for c in range(4)] + [f"usage:index16:{c}" for c in range(5)] + \
           ["usage_fresh", "usage_combined_across_images"] + [f"usage_bands:{n}" for n in (1, 2, 3)] + \
           ["s_usage_fresh", "s_usage_combined", "remap_in_place", "remap_planned_table", "remap_random_table", "bad_count_combined",
            "optimize_plan_bits", "optimize_given_bits", "optimize_path_replayed"]


def test_coverage_of_the_committed_seeds_of_surface_2(campaign_2):
    c = campaign_2["counters"]
    print({name: c[name] for name in coverage_names_2()}, campaign_2["ops"])
    assert not campaign_2["failures"]
    need = coverage_names_2()
    assert set(need) == set(EXACT_2), sorted(set(need) ^ set(EXACT_2))
    wrong = {name: (c[name], EXACT_2[name]) for name in need if c[name] != EXACT_2[name] or EXACT_2[name] < 1}
    assert not wrong, wrong
    assert all(n > 0 for seed in SEEDS_2 for n in campaign_2["reused"][seed])      # blocks re-used, in every sequence


# what the committed seeds of surface 3 give (SEEDS_3 x SEQUENCES), exactly, for what surface 3 adds.  None may be zero.
EXACT_3 = {
    'op:weight': 190, 'op:l_weight': 137, 'op:l_unbind': 12, 'op:motif': 73, 'refusal:weight_bad_value': 6,
    'refusal:l_weight_bad_value': 8, 'refusal:octree_weighted': 12, 'refusal:l_weight_under_caller_binding': 30,
    'refusal:weighted_bind': 18, 'refusal:weighted_lftu': 2, 'refusal:weighted_accumulate_into': 3,
    'refusal:weighted_no_kept_pixel': 15, 'motif:weight_cutoff': 11, 'motif:weight_adds': 12, 'motif:weight_warm': 11,
    'motif:weight_binding': 12, 'motif:weight_blocks': 11, 'motif:weight_fixed': 9, 'motif:weight_quality': 7,
    'l_weight:0:owner_nobody': 48, 'l_weight:0:owner_init': 12, 'l_weight:0:owner_caller': 14, 'l_weight:1:owner_nobody': 47,
    'l_weight:1:owner_init': 30, 'l_weight:1:owner_caller': 16, 'pass:l_assign:weighted': 16, 'pass:l_assign:unweighted': 34,
    'pass:l_assign_update:weighted': 42, 'pass:l_assign_update:unweighted': 68, 'pass:l_iterate:weighted': 9,
    'pass:l_iterate:unweighted': 3, 'pass:l_run:weighted': 33, 'pass:l_run:unweighted': 9, 'weighted_host:palette': 69,
    'weighted_host:reduce': 33, 'weighted_host:reduce_indexed': 68, 'weighted_host:quality': 13, 'weighted_host:optimize': 5,
    'octree_weighted:palette': 4, 'octree_weighted:reduce': 4, 'octree_weighted:reduce_indexed': 4,
    'weighted_no_kept_pixel:palette': 5, 'weighted_no_kept_pixel:reduce': 5, 'weighted_no_kept_pixel:reduce_indexed': 5,
    'weighted_host_at_cutoff_0': 105, 'host_call_on_the_map': 21, 'lloyd_pass_on_the_map': 74,
    'lloyd_object_created_right_after_a_weighted_one_closed': 31, 'free_cluster_of_weight_0_with_pixels': 12,
    'pinned_cluster_of_weight_0_with_pixels': 2, 'add_under_weighting': 50, 'add_under_weighting_loses_weight_0_pixels': 18,
    'sequence_loop_weighted': 49, 'sequence_loop_unweighted': 108, 'sequence_loop_weighting_differs_from_an_add': 37,
    'local_warm_weighted': 57, 'local_cold_weighted': 44, 'local_warm_weighting_differs_from_last_frame': 44,
    'quality_weighting_changes_the_palette': 6,
}


def coverage_names_3():
    """what surface 3 adds: every new op, refusal and motif; both binding owners crossed with both values of the Lloyd setter (under
    the caller's binding the call is the listed refusal); every pass of a Lloyd object and every palette call of the processor under
    weighting; the moments at which the switch is read"""
    return ["op:" + o for o in NEW_OPS_3] + ["refusal:" + r for r in H.REFUSALS_3] + ["motif:" + mo for mo in H.MOTIFS_3] + \
           [f"l_weight:{v}:owner_{who}" for v in (0, 1) for who in ("nobody", "init", "caller")] + \
           [f"pass:{p}:{w}" for p in ("l_assign", "l_assign_update", "l_iterate", "l_run") for w in ("weighted", "unweighted")] + \
           ["weighted_host:" + n for n in ("palette", "reduce", "reduce_indexed", "quality", "optimize")] + \
           [f"{r}:{call}" for r in ("octree_weighted", "weighted_no_kept_pixel") for call in ("palette", "reduce", "reduce_indexed")] + \
           ["weighted_host_at_cutoff_0", "host_call_on_the_map", "lloyd_pass_on_the_map", "lloyd_object_created_right_after_a_weighted_one_closed",
            "free_cluster_of_weight_0_with_pixels", "pinned_cluster_of_weight_0_with_pixels", "add_under_weighting",
            "add_under_weighting_loses_weight_0_pixels", "sequence_loop_weighted", "sequence_loop_unweighted",
            "sequence_loop_weighting_differs_from_an_add", "local_warm_weighted", "local_cold_weighted",
            "local_warm_weighting_differs_from_last_frame", "quality_weighting_changes_the_palette"]


def test_coverage_of_the_committed_seeds_of_surface_3(campaign_3):
    c = campaign_3["counters"]
    print({name: c[name] for name in coverage_names_3()}, campaign_3["ops"])
    assert not campaign_3["failures"]
    need = coverage_names_3()
    assert set(need) == set(EXACT_3), sorted(set(need) ^ set(EXACT_3))
    wrong = {name: (c[name], EXACT_3[name]) for name in need if c[name] != EXACT_3[name] or EXACT_3[name] < 1}
    assert not wrong, wrong
    assert all(n > 0 for seed in SEEDS_3 for n in campaign_3["reused"][seed])      # blocks re-used, in every sequence


# what the committed seeds of surface 4 give (SEEDS_4 x SEQUENCES), exactly, for what surface 4 adds.  None may be zero.
EXACT_4 = {
    'op:b_palette': 101, 'op:b_reduce': 76, 'op:b_reduce_indexed': 124, 'op:b_find': 98, 'op:b_palette_device': 65,
    'op:b_apply_device': 74, 'refusal:batch_fixed': 30, 'refusal:batch_weighted': 28, 'refusal:batch_no_kept_pixel': 22,
    'refusal:batch_index8_full': 3, 'refusal:batch_meld_indexed': 3, 'refusal:batch_bad_tables': 3, 'refusal:batch_empty': 3,
    'motif:batch_shrinking': 9, 'motif:batch_device_blocks': 11, 'motif:batch_cutoff': 12, 'motif:batch_switches': 9,
    'motif:batch_no_kept_pixel': 10, 'motif:batch_beside_objects': 10, 'motif:batch_octree': 9, 'bound:0': 254, 'bound:1': 89,
    'bound:pairs': 56, 'bound_cuts': 134, 'bound_pairs_cuts_twice': 44, 'batch_len:1': 42, 'batch_len:2': 132, 'batch_len:3+':
    364, 'batch_repeated_image': 226, 'batch_output:rgba8:replace': 17, 'batch_output:rgba8:dither': 25,
    'batch_output:index8:replace': 48, 'batch_output:index8:dither': 122, 'batch_output:index16:replace': 16,
    'batch_output:index16:dither': 43, 'batch_fixed:b_palette': 9, 'batch_fixed:b_reduce': 9, 'batch_fixed:b_reduce_indexed':
    12, 'batch_weighted:b_palette': 10, 'batch_weighted:b_reduce': 9, 'batch_weighted:b_reduce_indexed': 9,
    'batch_no_kept_pixel:b_palette': 8, 'batch_no_kept_pixel:b_reduce': 9, 'batch_no_kept_pixel:b_reduce_indexed': 5,
    'batch_no_kept_pixel:bound_0': 11, 'batch_no_kept_pixel:bound_1': 11, 'batch_octree': 27, 'batch_kmeans': 274,
    'batch_under_cutoff': 188, 'batch_under_forced_table': 327, 'tables:shared': 33, 'tables:per_image': 41,
    'batch_iterations_differ': 34, 'batch_offset:0': 24, 'batch_offset:4': 22, 'batch_offset:1': 28, 'batch_k:0': 9,
    'batch_k:1': 206, 'batch_k:2': 60, 'batch_k:3': 5, 'batch_k:4': 21,
}


def coverage_names_4():
    """what surface 4 adds: every batched op, refusal and motif; every class of max_resident_bytes, and that the computed bound did
    cut; every output format with replace and with dither; lists of one, two and more images and an image twice in a list; the
    refusals by call; k-means and octree batches, under a cutoff and under the forced table strategy; shared and per-image tables
    at every element offset; every class of k; batches whose images stop at different iterations"""
    return ["op:" + o for o in NEW_OPS_4] + ["refusal:" + r for r in H.REFUSALS_4] + ["motif:" + mo for mo in H.MOTIFS_4] + \
           ["bound:0", "bound:1", "bound:pairs", "bound_cuts", "bound_pairs_cuts_twice", "batch_len:1", "batch_len:2", "batch_len:3+", "batch_repeated_image"] + \
           [f"batch_output:{f}:{mo}" for f in ("rgba8", "index8", "index16") for mo in ("replace", "dither")] + \
           [f"{r}:{call}" for r in ("batch_fixed", "batch_weighted", "batch_no_kept_pixel") for call in H.BATCH_PALETTE_CALLS] + \
           ["batch_no_kept_pixel:bound_0", "batch_no_kept_pixel:bound_1", "batch_octree", "batch_kmeans", "batch_under_cutoff",
            "batch_under_forced_table", "tables:shared", "tables:per_image", "batch_iterations_differ"] + \
           [f"batch_offset:{o}" for o in H.CPAIR_OFFSETS] + [f"batch_k:{c}" for c in range(5)]


def test_coverage_of_the_committed_seeds_of_surface_4(campaign_4):
    c = campaign_4["counters"]
    print({name: c[name] for name in coverage_names_4()}, campaign_4["ops"])
    assert not campaign_4["failures"]
    need = coverage_names_4()
    assert set(need) == set(EXACT_4), sorted(set(need) ^ set(EXACT_4))
    wrong = {name: (c[name], EXACT_4[name]) for name in need if c[name] != EXACT_4[name] or EXACT_4[name] < 1}
    assert not wrong, wrong
    assert EXACT_4["bound_pairs_cuts_twice"] >= 12                                 # the computed bound cuts a list in three pieces or more: often
    assert all(n > 0 for seed in SEEDS_4 for n in campaign_4["reused"][seed])      # blocks re-used, in every sequence
