"""Command line driver with the reference CLI's sub-commands, flags, validation and output naming
(cli/src/args.rs:11-216, cli/src/main.rs:46-239), on top of libkmeans_hip.

    python -m kmeans_gpu_amd.cli reduce  -i img.png -c 8 [-a kmeans|octree] [-m replace|dither|meld|diffuse] [-o out.png]
    python -m kmeans_gpu_amd.cli find    -i img.png -p "#050505,#ffffff,#ff0000"|palette.png [-m ...] [-o out.png]
    python -m kmeans_gpu_amd.cli palette -i img.png -c 8 [-a ...] [-s 40] [-o out.png]
    python -m kmeans_gpu_amd.cli batch   -i A.png B.png ... -c 8 [-a ...] [-m ...] -o DIR [--indexed] | --palette

Every sub-command also takes `--alpha-cutoff N` (0..255, default 0 = alpha ignored, as in the reference): with N >= 1 only the
pixels whose alpha is at least N shape the palette, and the output keeps the input's alpha (include/kmeans_hip.h, kmg_options).

`find`, `reduce`, `sequence` and `batch` take `--diffusion NAME` with `-m diffuse`: the error-diffusion filter (floyd-steinberg, the
default; sierra-lite, atkinson, burkes, sierra2, sierra3, jarvis, stucki; include/kmeans_hip.h at kmg_diffusion).

`find`, `reduce`, `sequence` and `batch` take `--dither-map bayer2|bayer4|bayer8|bayer16|blue|FILE.png` and `--dither-strength S` with
`-m dither`: the threshold map of the ordered dither (bayer4, the reference's matrix, is the default; blue is a 64 x 64 blue-noise
map; a file is a grey 8-bit PNG whose sides are powers of two up to 64, its grey values the levels out of 256) and the factor
0 .. 4 on the dither's amplitude (default 1; include/kmeans_hip.h at kmg_dither_map).  Not with --devices.

`reduce` and `find` also take `--indexed`: the output is a palette-mode PNG (one index per pixel, PLTE = the palette; at most 256
colours) instead of RGBA.  In alpha mode the pixels below the cutoff take one more, fully transparent entry (tRNS 0), so
255 colours at most.

`reduce` and `find` also take `--report`: after the call one line with the error of the output against the input (pixels counted,
per-channel MSE, PSNR, dE76 RMS and max; kmg_compare).  `reduce --max-error DE [--min-colors A]` picks the colour count itself: as
few colours between A (default 2) and `-c` as keep the dE76 RMS of the palette step's working image at or below DE
(kmg_reduce_quality, k-means only); the line then also gives the count chosen and whether the target was reached.
`batch --max-error DE [--min-colors A]` does the same for every input of a batch in one call (kmg_reduce_quality_batch).

`reduce` and `find` with `--indexed` also take `--optimize [usage|luma|keep]` (kmg_index_optimize): the palette loses the entries
no pixel uses, is ordered by descending use (the default), ascending luma or as it was, the transparent slot of alpha mode comes
first (tRNS is then one byte), and the PNG is written at the bit depth the entries left need: 1, 2, 4 or 8 (kmeans_gpu_amd/png8.py).
`--report` compares before the rewrite.  `sequence --optimize` counts the use of every entry over all frames, drops the unused
ones, orders the rest by use (the transparent slot stays last, where the APNG wants it) and rewrites every map at 8 bits.

`sequence -i A.png B.png ... -c K [-m replace|dither|diffuse] [-o out.png] [--alpha-cutoff T] [--no-delta] [--lossy DE] [--report]
[--delay-ms 100]` quantises several frames of one size with ONE palette (kmg_sequence_*) and writes a palette-mode APNG
(kmeans_gpu_amd/apng.py): delta frames -- the rectangle of the pixels that changed, blended "over" -- unless --no-delta asks for
full frames.  K <= 255: the transparent slot takes the last palette entry.  `--lossy DE` (a dE76 distance >= 0) makes the delta
frames lossy (kmg_sequence_output_frame_lossy with tolerance = rint(4096 DE^2)): a pixel whose source stays within DE of the source it
was last written for keeps what it shows, so noise and dither flicker no longer fill the delta frames; not with --no-delta.
`--report` prints the changed (and held) pixels of every frame.  `--local` gives every frame a palette of its own
(Sequence.frame_local) and writes a GIF with local colour tables (kmeans_gpu_amd/gif.py) instead; `--warm` starts each frame's k-means
from the previous frame's centroids.  It composes with --lossy, --report, --no-delta and --fixed (--fixed not with --warm), not with
--optimize; with --alpha-cutoff every frame is written in full with disposal 2 (a full frame holds nothing: --lossy then has no
effect).

`palette`, `reduce` and `sequence` also take `--fixed "#RRGGBB,..."|palette.png` (the palette syntax of `find`): colours the k-means
palette keeps exactly, as its first entries in index order (the PLTE of `--indexed` and of `sequence`), while the other entries
are placed around them (kmg_processor_set_fixed_colors).  `-c` counts them; k-means only.

`palette`, `reduce` and `sequence` also take `--alpha-weight`: the k-means palette weighs every pixel by its alpha byte, so an
anti-aliased edge at alpha 20 pulls a colour a twelfth as hard as a solid pixel, and pixels of alpha 0 not at all
(kmg_processor_set_weighting; k-means only, not with --devices).  `--weights MAP.png` gives the weights as a greyscale image of the
input's size instead -- an importance map for an opaque image: 255 where the colours matter most, 0 where they do not matter at
all.  It implies --alpha-weight, replaces the input's alpha (the output is opaque) and is therefore refused together with a
non-zero --alpha-cutoff; `sequence` applies the one map to every frame.

`batch` reduces many images in one call (kmg_reduce_batch: one launch chain for the palettes of all of them, the results of
`reduce` image by image) and writes DIR/<name>-reduce-c<K>-<algo>-<mode>.png for every input; `--palette` prints their palettes
instead (kmg_palette_batch).  It takes --alpha-cutoff; not --fixed, --alpha-weight or --devices.
`batch --indexed` writes one palette-mode PNG per input instead (kmg_reduce_indexed_batch: the output passes of the images in one
launch as well; kmeans_gpu_amd/png8.py, 8 bits per pixel, the transparent slot of --alpha-cutoff as entry 0) and prints both reports.

Image decoding/encoding (the `image` crate in the reference) is done with Pillow.  One flag the reference does not have:
`--devices 0,1,...` (before the sub-command) runs the same operation over several GPUs of the node (kmg_group_*: the image
tiled in row bands, same bytes).
"""
import argparse
import os
import re
import sys
import time

import numpy as np

from . import DIFFUSION_NAMES, DITHER_MAP_NAMES, Algorithm, Group, ImageProcessor, ReduceMode

_PALETTE_RE = re.compile(r"^#[0-9a-fA-F]{6}(?:,#[0-9a-fA-F]{6})*$")     # args.rs:184
_MODES = {"replace": ReduceMode.Replace, "dither": ReduceMode.Dither, "meld": ReduceMode.Meld, "diffuse": ReduceMode.Diffuse}
_ALGOS = {"kmeans": Algorithm.Kmeans, "octree": Algorithm.Octree}


def validate_k(s):                                       # args.rs:160-171
    try:
        k = int(s)
    except ValueError:
        k = 0
    if k < 1:
        raise argparse.ArgumentTypeError("k must be an integer higher than 0.")
    return k


def validate_filename(s):                                # args.rs:173-179
    if len(s) > 4 and (s.endswith(".png") or s.endswith(".jpg")):
        return s
    raise argparse.ArgumentTypeError("Only support png or jpg files.")


def validate_sequence_output(s):
    """`sequence -o`: what validate_filename takes, and a .gif for --local (which of them fits is checked once --local is known)"""
    if len(s) > 4 and s.endswith(".gif"):
        return s
    return validate_filename(s)


def parse_colors(s):                                     # args.rs:218-231
    return np.array([[int(c[1:3], 16), int(c[3:5], 16), int(c[5:7], 16), 255] for c in s.split(",")], np.uint8)


def parse_palette(path):                                 # args.rs:197-216
    from PIL import Image
    px = np.array(Image.open(path).convert("RGBA")).reshape(-1, 4)
    if px.shape[0] > 512:
        raise argparse.ArgumentTypeError("Trying to load a palette with more than 512 colors")
    colors = sorted(set(map(tuple, px)))
    if len(colors) < px.shape[0]:
        raise argparse.ArgumentTypeError("Trying to load a palette with recuring colors")
    return np.array(colors, np.uint8)


def validate_palette(s):                                 # args.rs:181-195
    if _PALETTE_RE.match(s):
        return parse_colors(s)
    if len(s) > 4 and (s.endswith(".png") or s.endswith(".jpg")) and os.path.exists(s):
        return parse_palette(s)
    raise argparse.ArgumentTypeError('The palette should be a path to an image file, or defined as "#RRGGBB,#RRGGBB,#RRGGBB"')


def _load(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGBA"))      # image::open(..).to_rgba8()


def _load_weights(path, width, height, ap):
    """`--weights`: a greyscale map of the input's size as (height, width) uint8; anything else ends the command"""
    from PIL import Image
    w = np.array(Image.open(path).convert("L"))
    if w.shape != (height, width):
        ap.error(f"--weights: {path} is {w.shape[1]}x{w.shape[0]}, the input is {width}x{height}")
    return w


def _save(path, rgba):
    from PIL import Image
    Image.fromarray(rgba, "RGBA").save(path)


def save_indexed(path, palette, index, transparent=False):
    """A palette-mode PNG: `index` (height, width) into `palette` (n, 4); transparent: index n is a fully transparent slot (PLTE
    entry n black, tRNS 0 for it and 255 for the colours)"""
    from PIL import Image
    pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)[:, :3]
    n = pal.shape[0] + (1 if transparent else 0)
    if n > 256:
        raise ValueError(f"a palette PNG holds 256 entries, {n} needed")
    img = Image.fromarray(np.ascontiguousarray(index, np.uint8), "P")
    plte = np.zeros((n, 3), np.uint8)
    plte[:pal.shape[0]] = pal
    img.putpalette(plte.reshape(-1).tolist(), rawmode="RGB")
    if transparent:
        img.save(path, transparency=bytes([255] * pal.shape[0] + [0]))
    else:
        img.save(path)


_ORDERS = {"usage": 1, "luma": 2, "keep": 0}                 # KMG_INDEX_ORDER_*


def save_optimized(proc, path, palette, index, order):
    """--indexed --optimize: the palette pruned and ordered, the transparent slot first, the PNG at the plan's bit depth"""
    from . import INDEX_TRANSPARENT_FIRST, png8
    colors, rows, info = proc.optimize_indexed(index, palette, _ORDERS[order] | INDEX_TRANSPARENT_FIRST)
    h, w = np.asarray(index).shape
    png8.write(path, colors, w, h, rows, info.bits, transparent_first=info.transparent == 0)
    print(f"Optimized: {info.n_colors} of {np.asarray(palette).reshape(-1, 4).shape[0]} colours used"
          + (", transparent slot first" if info.transparent == 0 else "") + f", {info.bits} bits per pixel")


def reduce_file_path(k, algo, mode, output, inp):        # main.rs:127-153
    if output:
        return output
    stem = os.path.splitext(os.path.basename(inp))[0]
    return os.path.join(os.path.dirname(inp), f"{stem}-reduce-c{k}-{algo}-{mode}.png")


def palette_file_path(k, inp, output, algo, size):       # main.rs:155-182
    if output:
        return output
    stem = os.path.splitext(os.path.basename(inp))[0]
    return os.path.join(os.path.dirname(inp), f"{stem}-palette-c{k}-{algo}-s{size}.png")


def find_file_path(mode, output, inp):                   # main.rs:184-219
    if output:
        return output
    stem, ext = os.path.splitext(os.path.basename(inp))
    millis = int(time.time() * 1000)
    return os.path.join(os.path.dirname(inp), f"{stem}-find-{mode}-{millis}{ext}")


def sequence_file_path(k, mode, output, inp, ext=".png"):
    if output:
        return output
    stem = os.path.splitext(os.path.basename(inp))[0]
    return os.path.join(os.path.dirname(inp), f"{stem}-sequence-c{k}-{mode}{ext}")


def validate_delay(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid value '{s}': not an integer")
    if not 0 <= v <= 65535:
        raise argparse.ArgumentTypeError(f"{v} is not in 0..=65535")
    return v


def run_sequence_local(args, frames, w, h, out_path):
    """`sequence --local`: every input gets a palette of its own (Sequence.frame_local); a GIF with local colour tables"""
    from . import OutputFormat, gif
    delay = (args.delay_ms + 5) // 10
    coded, n_full, n_changed, n_held, lines = [], 0, 0, 0, []
    # alpha mode: GIF cannot clear the whole canvas from a small rectangle, so every frame is written in full, disposal 2 -- and a
    # frame that is not a delta frame holds nothing: --lossy then has no effect
    delta = not (args.no_delta or args.alpha_cutoff)
    lossy = args.lossy if delta else None
    with ImageProcessor(alpha_cutoff=args.alpha_cutoff, fixed_colors=args.fixed, alpha_weight=args.alpha_weight,
                        diffusion=args.diffusion or 0) as proc, proc.sequence() as seq:
        _set_dither(proc, args)
        seq.output_local(args.colorcount, _MODES[args.mode], OutputFormat.Index8, w, h, warm=args.warm)
        for i, f in enumerate(frames):
            index, colors, info, is_full = seq.frame_local(f, delta=delta, tolerance=lossy)
            rect = None if is_full else (info.rect or (0, 0, 1, 1))           # (nothing changed: one transparent pixel)
            coded.append({"indices": index, "palette": colors, "rect": rect, "delay": delay, "disposal": 2 if args.alpha_cutoff else 1})
            n_full += 1 if is_full else 0
            n_changed += int(info.changed)
            line = f"Frame {i}: changed={int(info.changed)}"
            if lossy is not None:
                n_held += int(info.held)
                line += f" held={int(info.held)} held dE76 rms={info.held_delta_e_rms:.3f}"
            lines.append(line + (" (written in full)" if is_full else ""))
        seq.end_output()
    gif.write(out_path, w, h, coded)
    print(f"Sequence: {len(frames)} frames of {w}x{h} with a palette each, {n_full} written in full"
          + (f", {n_changed} changed pixels in the delta frames" if delta else "")
          + ("" if lossy is None else f", {n_held} held") + f": {out_path}")
    if args.report:
        print("\n".join(lines))
    return 0


def run_sequence(args, ap):
    """the `sequence` sub-command: one palette over all inputs, then every input as a frame of a palette-mode APNG"""
    from . import OutputFormat, apng
    frames = [_load(path) for path in args.input]
    h, w = frames[0].shape[:2]
    for path, f in zip(args.input, frames):
        if f.shape[:2] != (h, w):
            ap.error(f"every input of `sequence` must have one size: {path} is {f.shape[1]}x{f.shape[0]}, {args.input[0]} is {w}x{h}")
    out_path = sequence_file_path(args.colorcount, args.mode, args.output, args.input[0], ".gif" if args.local else ".png")
    if args.weights is not None:
        from . import with_weights
        weights = _load_weights(args.weights, w, h, ap)
        frames = [with_weights(f, weights) for f in frames]
    if args.local:
        return run_sequence_local(args, frames, w, h, out_path)
    with ImageProcessor(alpha_cutoff=args.alpha_cutoff, fixed_colors=args.fixed, alpha_weight=args.alpha_weight,
                        diffusion=args.diffusion or 0) as proc, proc.sequence() as seq:
        _set_dither(proc, args)
        for f in frames:
            seq.add(f)
        colors = seq.output(args.colorcount, _MODES[args.mode], OutputFormat.Index8, w, h)
        coded, n_full, n_changed, n_held, lines = [], 0, 0, 0, []
        # the whole clip in one launch chain (Sequence.frames): frame by frame what Sequence.frame returns
        for i, (index, info, is_full) in enumerate(seq.frames(frames, delta=not args.no_delta, tolerance=args.lossy)):
            coded.append((index, info.rect, is_full))
            n_full += 1 if is_full else 0
            n_changed += int(info.changed)
            line = f"Frame {i}: changed={int(info.changed)}"
            if args.lossy is not None:
                n_held += int(info.held)
                line += f" held={int(info.held)} held dE76 rms={info.held_delta_e_rms:.3f}"
            lines.append(line + (" (written in full)" if is_full else ""))
        seq.end_output()
        if args.optimize:                                    # one plan over every frame's map; the slot stays last (apng.encode)
            from . import INDEX_KEEP_TRANSPARENT, INDEX_ORDER_USAGE, index_plan
            k = colors.shape[0]
            use = np.zeros(k + 2, np.uint64)
            for index, _, _ in coded:
                proc.index_usage(index, k, usage=use)
            remap, pruned, info = index_plan(use, colors, INDEX_ORDER_USAGE | INDEX_KEEP_TRANSPARENT)
            coded = [(proc.index_remap(index, k, remap, 8)[0], rect, is_full) for index, rect, is_full in coded]
            colors = pruned[:info.n_colors]
            print(f"Optimized: {info.n_colors} of {k} colours used")
    apng.write(out_path, colors, w, h, coded, delay_ms=args.delay_ms)
    print("Palette: " + ",".join(f"#{c[0]:02X}{c[1]:02X}{c[2]:02X}" for c in colors))
    print(f"Sequence: {len(frames)} frames of {w}x{h}, {n_full} written in full"
          + ("" if args.no_delta else f", {n_changed} changed pixels in the delta frames")
          + ("" if args.lossy is None else f", {n_held} held") + f": {out_path}")
    if args.report:
        print("\n".join(lines))
    return 0


def validate_size(s):                                       # args.rs:36-38 value_parser!(u32).range(1..=60)
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid value '{s}': not an integer")
    if not 1 <= v <= 60:
        raise argparse.ArgumentTypeError(f"{v} is not in 1..=60")
    return v


def validate_alpha_cutoff(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid value '{s}': not an integer")
    if not 0 <= v <= 255:
        raise argparse.ArgumentTypeError(f"{v} is not in 0..=255")
    return v


def validate_max_error(s):
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid value '{s}': not a number")
    if not 0.0 <= v <= 1000.0:
        raise argparse.ArgumentTypeError(f"{v} is not in 0..=1000")
    return v


def validate_lossy(s):
    """--lossy DE: a dE76 distance as the tolerance of the lossy delta frames, rint(4096 DE^2) as a uint32"""
    from . import tolerance_of
    try:
        return tolerance_of(float(s))
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"invalid value '{s}': {e}")


def report_line(stats, chosen=None, reached=None):
    """the one line of --report / --max-error (an ErrorStats of the output against the input)"""
    mse = stats.mse
    line = (f"Error: pixels={int(stats.pixels)} mse=({mse[0]:.3f},{mse[1]:.3f},{mse[2]:.3f}) psnr={stats.psnr:.2f}dB "
            f"dE76 rms={stats.delta_e_rms:.3f} max={stats.delta_e_max:.3f}")
    if chosen is not None:
        line += f" colors={chosen} target {'reached' if reached else 'not reached'}"
    return line


def validate_devices(s):
    try:
        devices = [int(v) for v in s.split(",")]
    except ValueError:
        devices = []
    if not devices or min(devices) < 0:
        raise argparse.ArgumentTypeError("--devices takes a comma separated list of device ordinals, e.g. 0,1")
    return devices


def build_parser():
    """the argument parser of every sub-command"""
    ap = argparse.ArgumentParser(prog="kmeans-hip", description="k-means colour quantisation on MI355X")
    ap.add_argument("--devices", type=validate_devices, default=None,
                    help="HIP device ordinals, e.g. 0,1,2,3: tile the image over several GPUs (no counterpart in the reference)")
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("palette", help="Create an image with the dominant colors of the input")
    p.add_argument("-c", "--colorcount", type=validate_k, required=True)
    p.add_argument("-i", "--input", type=validate_filename, required=True)
    p.add_argument("-o", "--output", type=validate_filename)
    p.add_argument("-a", "--algo", choices=list(_ALGOS), default="kmeans")
    p.add_argument("-s", "--size", type=validate_size, default=40)
    f = sub.add_parser("find", help="Replace the colors of the input with the closest ones of a palette")
    f.add_argument("-i", "--input", type=validate_filename, required=True)
    f.add_argument("-o", "--output", type=validate_filename)
    f.add_argument("-p", "--palette", type=validate_palette, required=True)
    f.add_argument("-m", "--mode", choices=list(_MODES), default="replace")
    r = sub.add_parser("reduce", help="Reduce the number of colors of the input")
    r.add_argument("-c", "--colorcount", type=validate_k, required=True)
    r.add_argument("-i", "--input", type=validate_filename, required=True)
    r.add_argument("-o", "--output", type=validate_filename)
    r.add_argument("-a", "--algo", choices=list(_ALGOS), default="kmeans")
    r.add_argument("-m", "--mode", choices=list(_MODES), default="replace")
    q = sub.add_parser("sequence", help="Reduce several frames of one size with one shared palette; writes a palette-mode APNG")
    q.add_argument("-c", "--colorcount", type=validate_k, required=True)
    q.add_argument("-i", "--input", type=validate_filename, nargs="+", required=True)
    q.add_argument("-o", "--output", type=validate_sequence_output)
    q.add_argument("-m", "--mode", choices=["replace", "dither", "diffuse"], default="replace")
    q.add_argument("--no-delta", action="store_true", help="write every frame in full instead of the rectangle of its changes")
    q.add_argument("--lossy", type=validate_lossy, default=None, metavar="DE",
                   help="lossy delta frames: a pixel whose source stays within dE76 DE of the source it was last written for keeps what it shows")
    q.add_argument("--optimize", action="store_true",
                   help="drop the palette entries no frame uses and order the rest by use (the transparent slot stays last)")
    q.add_argument("--report", action="store_true", help="print the changed (and, with --lossy, the held) pixels of every frame")
    q.add_argument("--local", action="store_true",
                   help="a palette per frame instead of one for all: writes a GIF with local colour tables (not with --optimize)")
    q.add_argument("--warm", action="store_true",
                   help="with --local: every frame's k-means starts from the previous frame's centroids (not with --fixed)")
    q.add_argument("--delay-ms", type=validate_delay, default=100, help="display time of every frame in milliseconds (default 100)")
    b = sub.add_parser("batch", help="Reduce many images with one launch chain for their palettes; one output per input")
    b.add_argument("-c", "--colorcount", type=validate_k, required=True)
    b.add_argument("-i", "--input", nargs="+", required=True)
    b.add_argument("-o", "--output", metavar="DIR", help="directory of the outputs (created if missing)")
    b.add_argument("-a", "--algo", choices=list(_ALGOS), default="kmeans")
    b.add_argument("-m", "--mode", choices=list(_MODES), default="replace")
    b.add_argument("--palette", action="store_true", help="print the palette of every input instead of writing reduced images")
    b.add_argument("--indexed", action="store_true",
                   help="write a palette-mode PNG (an index per pixel) per input instead of RGBA; at most 256 colours, 255 with --alpha-cutoff")
    b.add_argument("--max-error", type=validate_max_error, default=None, metavar="DE",
                   help="choose every image's colour count: as few colours (at most -c) as keep the dE76 RMS of its shrunk image at or "
                        "below DE; k-means only (kmg_reduce_quality_batch)")
    b.add_argument("--min-colors", type=validate_k, default=None, metavar="A", help="lower bound of --max-error's search (default 2)")
    for s in (p, f, r, q, b):
        s.add_argument("--alpha-cutoff", type=validate_alpha_cutoff, default=0,
                       help="1..255: pixels with a lower alpha do not shape the palette, the output keeps the input's alpha")
    for s in (f, r, q, b):
        s.add_argument("--diffusion", choices=list(DIFFUSION_NAMES), default=None, metavar="NAME",
                       help="with -m diffuse: the error-diffusion filter, one of " + ", ".join(DIFFUSION_NAMES) + " (default floyd-steinberg)")
    for s in (f, r, q, b):
        s.add_argument("--dither-map", default=None, metavar="MAP",
                       help="with -m dither: the threshold map, one of " + ", ".join(sorted(DITHER_MAP_NAMES)) + " (default bayer4, the "
                            "reference's matrix) or a grey 8-bit PNG with sides that are powers of two up to 64")
        s.add_argument("--dither-strength", type=validate_dither_strength, default=None, metavar="S",
                       help="with -m dither: a factor 0 .. 4 on the dither's amplitude (default 1)")
    for s in (p, r, q):
        s.add_argument("--fixed", type=validate_palette, default=None, metavar="COLORS",
                       help='"#RRGGBB,..." or a palette image: colours the k-means palette keeps exactly, as its first entries; -c counts them')
    for s in (p, r, q):
        s.add_argument("--alpha-weight", action="store_true",
                       help="the k-means palette weighs every pixel by its alpha byte (pixels of alpha 0 do not shape it at all)")
        s.add_argument("--weights", type=validate_filename, default=None, metavar="MAP",
                       help="a greyscale image of the input's size: the weight of every pixel, in place of its alpha; implies "
                            "--alpha-weight, not with a non-zero --alpha-cutoff")
    for s in (f, r):
        s.add_argument("--indexed", action="store_true",
                       help="write a palette-mode PNG (an index per pixel) instead of RGBA; at most 256 colours, 255 with --alpha-cutoff")
        s.add_argument("--optimize", nargs="?", const="usage", default=None, choices=list(_ORDERS), metavar="ORDER",
                       help="with --indexed: drop unused palette entries, order the rest (usage, the default; luma; keep), put the "
                            "transparent slot first and write the PNG at 1, 2, 4 or 8 bits per pixel")
        s.add_argument("--report", action="store_true",
                       help="print one line with the error of the output against the input: pixels, MSE per channel, PSNR, dE76 RMS and max")
    r.add_argument("--max-error", type=validate_max_error, default=None, metavar="DE",
                   help="choose the colour count: as few colours (at most -c) as keep the dE76 RMS of the shrunk image at or below DE; k-means only")
    r.add_argument("--min-colors", type=validate_k, default=None, metavar="A", help="lower bound of --max-error's search (default 2)")
    return ap


def check_diffusion(args, ap):
    """--diffusion names the filter of -m diffuse: an argument error with any other mode"""
    if getattr(args, "diffusion", None) is not None and args.mode != "diffuse":
        ap.error("--diffusion names the filter of -m diffuse: it needs -m diffuse")


def validate_dither_strength(s):
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s} is not a number")
    if not (np.isfinite(v) and 0.0 <= v <= 4.0):
        raise argparse.ArgumentTypeError(f"{s} is not in 0..=4")
    return v


def check_dither(args, ap):
    """--dither-map and --dither-strength belong to -m dither: an argument error with any other mode.  Leaves args.dither = None
    (the default) or (map, strength, levels) as ImageProcessor.set_dither takes them"""
    name, strength = getattr(args, "dither_map", None), getattr(args, "dither_strength", None)
    args.dither = None
    if name is None and strength is None:
        return
    if args.mode != "dither":
        ap.error("--dither-map and --dither-strength shape the ordered dither: they need -m dither")
    if getattr(args, "devices", None):
        ap.error("--dither-map and --dither-strength are not supported with --devices")
    if name is None or name.lower() in DITHER_MAP_NAMES:
        args.dither = ((name or "bayer4").lower(), 1.0 if strength is None else strength, None)
        return
    if not name.lower().endswith(".png"):
        ap.error(f"--dither-map: {name} is neither one of {', '.join(sorted(DITHER_MAP_NAMES))} nor a PNG file")
    from PIL import Image
    try:
        im = Image.open(name)
        im.load()
    except OSError as e:
        ap.error(f"--dither-map: cannot read {name}: {e}")
    if im.mode != "L":
        ap.error(f"--dither-map: {name} is not a grey 8-bit PNG (mode {im.mode})")
    w, h = im.size
    if any(v < 1 or v > 64 or v & (v - 1) for v in (w, h)):
        ap.error(f"--dither-map: {name} is {w}x{h}; each side must be a power of two up to 64")
    args.dither = (np.asarray(im, np.uint8).astype(np.uint16), 1.0 if strength is None else strength, 256)


def _set_dither(proc, args):
    if args.dither is not None:
        proc.set_dither(args.dither[0], args.dither[1], levels=args.dither[2])
    return proc


def run_batch(args, ap):
    """the `batch` sub-command: every input through one kmg_reduce_batch (or, --palette, kmg_palette_batch; --indexed,
    kmg_reduce_indexed_batch; --max-error, kmg_reduce_quality_batch) call"""
    if args.devices:
        ap.error("`batch` is not supported with --devices")
    if args.max_error is not None:
        if args.algo != "kmeans":
            ap.error("--max-error searches the k-means colour count: -a octree has no such knob")
        if args.palette:
            ap.error("--max-error writes images: not with --palette")
        if args.min_colors is None:
            args.min_colors = min(2, args.colorcount)
        if args.min_colors > args.colorcount:
            ap.error(f"--min-colors {args.min_colors} is above -c {args.colorcount}")
    elif args.min_colors is not None:
        ap.error("--min-colors belongs to --max-error")
    if not args.palette and not args.output:
        ap.error("`batch` writes one output per input: it needs -o DIR (or --palette)")
    if args.indexed:
        limit = 255 if args.alpha_cutoff else 256
        if args.palette:
            ap.error("--indexed writes images: not with --palette")
        if args.mode == "meld":
            ap.error("--indexed has no meld mode: meld blends two colours, so a pixel has no palette index")
        if args.colorcount > limit:
            ap.error(f"--indexed writes a palette PNG of at most {limit} colours{' (plus the transparent slot)' if args.alpha_cutoff else ''}; "
                     f"{args.colorcount} requested")
    images = [_load(path) for path in args.input]
    with ImageProcessor(alpha_cutoff=args.alpha_cutoff, diffusion=args.diffusion or 0) as proc:
        _set_dither(proc, args)
        if args.max_error is not None:                   # every image's colour count from the quality target; -c is the upper bound
            os.makedirs(args.output, exist_ok=True)
            results = proc.reduce_quality_batch(images, args.max_error, args.min_colors, args.colorcount, _MODES[args.mode], indexed=args.indexed)
            for path, (k, colors, out, _, reached) in zip(args.input, results):
                name = os.path.basename(reduce_file_path(args.colorcount, args.algo, args.mode, None, path))
                if args.indexed:
                    save_indexed(os.path.join(args.output, os.path.splitext(name)[0] + ".png"), colors, out, transparent=bool(args.alpha_cutoff))
                else:
                    _save(os.path.join(args.output, name), out)
                print(f"Quality {path}: {k} colours, target {'reached' if reached else 'not reached'}")
            qrep = proc.last_quality_report
            print(f"Batch quality: {len(images)} images, {qrep.rounds} rounds, {qrep.palette_runs} palette runs, {qrep.launches} + "
                  f"{qrep.measure_launches} launches, output {qrep.batched} batched and {qrep.per_image} per image, {qrep.sub_batches} sub-batches, "
                  f"{qrep.fallback} on the per-image path")
            return 0
        if args.palette:
            for path, colors in zip(args.input, proc.palette_batch(args.colorcount, images, _ALGOS[args.algo])):
                print(f"Palette {path}: " + ",".join(f"#{c[0]:02X}{c[1]:02X}{c[2]:02X}" for c in colors))
        elif args.indexed:
            from . import png8
            os.makedirs(args.output, exist_ok=True)
            pairs = proc.reduce_indexed_batch(args.colorcount, images, _ALGOS[args.algo], _MODES[args.mode])
            for path, (colors, index) in zip(args.input, pairs):
                name = os.path.splitext(os.path.basename(reduce_file_path(args.colorcount, args.algo, args.mode, None, path)))[0] + ".png"
                if args.alpha_cutoff:
                    # the transparent slot (index len(colors)) becomes entry 0, which is where png8 writes its one tRNS byte
                    colors = np.concatenate([np.zeros((1, 4), np.uint8), colors])
                    index = ((index.astype(np.uint16) + 1) % len(colors)).astype(np.uint8)
                png8.write(os.path.join(args.output, name), colors, index.shape[1], index.shape[0], index, 8,
                           transparent_first=bool(args.alpha_cutoff))
            arep = proc.last_batch_apply_report
            print(f"Batch output: {arep.launches} launches for {arep.batched} images, {arep.per_image} on the per-image pass, "
                  f"{arep.sub_batches} sub-batches")
        else:
            os.makedirs(args.output, exist_ok=True)
            outs = proc.reduce_batch(args.colorcount, images, _ALGOS[args.algo], _MODES[args.mode])
            for path, out in zip(args.input, outs):
                name = os.path.basename(reduce_file_path(args.colorcount, args.algo, args.mode, None, path))
                _save(os.path.join(args.output, name), out)
        rep = proc.last_batch_report
        print(f"Batch: {len(images)} images, {rep.launches} launches, {rep.iterations} iterations at most, {rep.sub_batches} sub-batches, "
              f"{rep.fallback} on the per-image path")
    return 0


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_diffusion(args, ap)
    check_dither(args, ap)
    if args.command == "batch":
        return run_batch(args, ap)
    if getattr(args, "weights", None) is not None:
        if args.alpha_cutoff:
            ap.error("--weights replaces the input's alpha with the map: it cannot be combined with a non-zero --alpha-cutoff")
        args.alpha_weight = True
    if getattr(args, "alpha_weight", False):
        if args.devices:
            ap.error("--alpha-weight is not supported with --devices")
        if getattr(args, "algo", "kmeans") != "kmeans":
            ap.error("--alpha-weight weighs the sums of the k-means palette: -a octree has none")
    fixed = getattr(args, "fixed", None)
    if fixed is not None:
        if args.devices:
            ap.error("--fixed is not supported with --devices")
        if getattr(args, "algo", "kmeans") != "kmeans":
            ap.error("--fixed pins entries of the k-means palette: -a octree has none")
        lowest = args.min_colors if getattr(args, "min_colors", None) is not None else args.colorcount
        if fixed.shape[0] > lowest:
            ap.error(f"--fixed names {fixed.shape[0]} colours, more than the {lowest} the palette may have")
    if args.command == "sequence":
        if args.devices:
            ap.error("`sequence` is not supported with --devices")
        if args.lossy is not None and args.no_delta:
            ap.error("--lossy makes the delta frames lossy: it cannot be combined with --no-delta")
        if args.colorcount > 255:
            ap.error(f"`sequence` writes a palette APNG of at most 255 colours plus the transparent slot; {args.colorcount} requested")
        if args.warm and not args.local:
            ap.error("--warm starts a frame's palette from the previous frame's: it needs --local")
        if args.local and args.optimize:
            ap.error("--local writes every frame's own palette: it cannot be combined with --optimize")
        if args.warm and fixed is not None:
            ap.error("--warm moves every centroid: it cannot be combined with --fixed")
        out_path = sequence_file_path(args.colorcount, args.mode, args.output, args.input[0], ".gif" if args.local else ".png")
        if args.local and not out_path.endswith(".gif"):
            ap.error("`sequence --local` writes a GIF file")
        if not args.local and out_path.endswith(".gif"):
            ap.error("argument -o/--output: Only support png or jpg files.")
        if not args.local and not out_path.endswith(".png"):
            ap.error("`sequence` writes a PNG file")
        return run_sequence(args, ap)
    if args.devices and args.alpha_cutoff:
        ap.error("--alpha-cutoff is not supported with --devices")
    report = getattr(args, "report", False)
    max_error = getattr(args, "max_error", None)
    if report and args.devices:
        ap.error("--report is not supported with --devices")
    if max_error is not None:
        if args.devices:
            ap.error("--max-error is not supported with --devices")
        if args.algo != "kmeans":
            ap.error("--max-error searches the k-means colour count: -a octree has no such knob")
        if args.min_colors is None:
            args.min_colors = min(max(2, fixed.shape[0] if fixed is not None else 0), args.colorcount)
        if args.min_colors > args.colorcount:
            ap.error(f"--min-colors {args.min_colors} is above -c {args.colorcount}")
    elif getattr(args, "min_colors", None) is not None:
        ap.error("--min-colors belongs to --max-error")
    indexed = getattr(args, "indexed", False)
    optimize = getattr(args, "optimize", None)
    if optimize is not None and not indexed:
        ap.error("--optimize rewrites an index map: it needs --indexed")
    if indexed:
        n = args.colorcount if args.command == "reduce" else args.palette.shape[0]
        limit = 255 if args.alpha_cutoff else 256
        if args.devices:
            ap.error("--indexed is not supported with --devices")
        if args.mode == "meld":
            ap.error("--indexed has no meld mode: meld blends two colours, so a pixel has no palette index")
        if n > limit:
            ap.error(f"--indexed writes a palette PNG of at most {limit} colours{' (plus the transparent slot)' if args.alpha_cutoff else ''}; "
                     f"{n} requested")
        out_path = (reduce_file_path(args.colorcount, args.algo, args.mode, args.output, args.input) if args.command == "reduce"
                    else find_file_path(args.mode, args.output, args.input))
        if not out_path.endswith(".png"):
            ap.error("--indexed writes a PNG file")

    image = _load(args.input)
    if getattr(args, "weights", None) is not None:
        from . import with_weights
        image = with_weights(image, _load_weights(args.weights, image.shape[1], image.shape[0], ap))
    if args.devices:
        proc = Group(devices=args.devices)
    else:
        options = {}                                     # (only what the command line asks for)
        if args.alpha_cutoff:
            options["alpha_cutoff"] = args.alpha_cutoff
        if fixed is not None:
            options["fixed_colors"] = fixed
        if getattr(args, "alpha_weight", False):
            options["alpha_weight"] = True
        if getattr(args, "diffusion", None) is not None:
            options["diffusion"] = args.diffusion
        proc = _set_dither(ImageProcessor(**options), args)
    with proc:
        if args.command == "palette":                    # main.rs:46-72
            colors = proc.palette(args.colorcount, image, _ALGOS[args.algo])
            out = np.repeat(np.repeat(colors[None, :, :], args.size, axis=0), args.size, axis=1)   # main.rs:221-239
            _save(palette_file_path(args.colorcount, args.input, args.output, args.algo, args.size), out)
            print("Palette: " + ",".join(f"#{c[0]:02X}{c[1]:02X}{c[2]:02X}" for c in colors))
        elif indexed and args.command == "find":
            index = proc.find_indexed(image, args.palette, _MODES[args.mode])
            if optimize is not None:
                save_optimized(proc, out_path, args.palette, index, optimize)
            else:
                save_indexed(out_path, args.palette, index, transparent=bool(args.alpha_cutoff))
            if report:
                print(report_line(proc.compare(image, index, palette=args.palette)))
        elif max_error is not None:                      # the colour count from the quality target; -c is the upper bound
            k, colors, out, _, reached = proc.reduce_quality(image, max_error, args.min_colors, args.colorcount, _MODES[args.mode],
                                                             indexed=indexed)
            if indexed and optimize is not None:
                save_optimized(proc, out_path, colors, out, optimize)
            elif indexed:
                save_indexed(out_path, colors, out, transparent=bool(args.alpha_cutoff))
            else:
                _save(reduce_file_path(args.colorcount, args.algo, args.mode, args.output, args.input), out)
            print(report_line(proc.compare(image, out, palette=colors if indexed else None), chosen=k, reached=reached))
        elif indexed:
            colors, index = proc.reduce_indexed(args.colorcount, image, _ALGOS[args.algo], _MODES[args.mode])
            if optimize is not None:
                save_optimized(proc, out_path, colors, index, optimize)
            else:
                save_indexed(out_path, colors, index, transparent=bool(args.alpha_cutoff))
            if report:
                print(report_line(proc.compare(image, index, palette=colors)))
        elif args.command == "find":                     # main.rs:74-98
            out = proc.find(image, args.palette, _MODES[args.mode])
            _save(find_file_path(args.mode, args.output, args.input), out)
            if report:
                print(report_line(proc.compare(image, out)))
        else:                                            # main.rs:100-125
            out = proc.reduce(args.colorcount, image, _ALGOS[args.algo], _MODES[args.mode])
            _save(reduce_file_path(args.colorcount, args.algo, args.mode, args.output, args.input), out)
            if report:
                print(report_line(proc.compare(image, out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
