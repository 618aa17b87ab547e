"""The surface of the error statistics and of the quality-targeted colour count, without a device: the new symbols of
include/kmeans_hip.h are exported, kmg_error_stats is 14 x uint64, the argument refusals that need no device come back as
KMG_ERR_INVALID_ARGUMENT with their own message, and the Python package and the command line carry the feature."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("kmg_dev_compare", "kmg_compare", "kmg_reduce_quality")


def test_new_symbols_are_declared_and_exported():
    import kmeans_gpu_amd as kg
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    L = C.CDLL(kg.library_path())
    for name in NEW:
        assert re.search(r"KMG_API\s+int\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
        assert name in kg.SYMBOLS
    assert re.search(r"#define\s+KMG_ERROR_RGB\s+1u", header) and re.search(r"#define\s+KMG_ERROR_LAB\s+2u", header)
    assert (kg.ERROR_RGB, kg.ERROR_LAB) == (1, 2)
    blob = open(kg.library_path(), "rb").read()
    assert b"k_error_stats" in blob and b"k_error_palette" in blob          # the gfx950 kernels of csrc/kmg_error.hip


def test_struct_is_14_uint64_without_padding():
    import kmeans_gpu_amd as kg
    assert C.sizeof(kg.ErrorStats) == 112
    names = [n for n, _ in kg.ErrorStats._fields_]
    assert names == ["pixels", "changed", "invalid", "sse", "sad", "max_abs", "lab_sse", "lab_max"]
    offsets = [getattr(kg.ErrorStats, n).offset for n in names]
    assert offsets == [0, 8, 16, 24, 48, 72, 96, 104]
    header = open(os.path.join(ROOT, "include", "kmeans_hip.h")).read()
    body = re.search(r"typedef struct kmg_error_stats \{(.*?)\} kmg_error_stats;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = re.findall(r"uint64_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [(n, int(c or 1)) for n, c in fields] == [("pixels", 1), ("changed", 1), ("invalid", 1), ("sse", 3), ("sad", 3),
                                                      ("max_abs", 3), ("lab_sse", 1), ("lab_max", 1)]
    s = kg.ErrorStats.from_array(np.arange(14, dtype=np.uint64))
    assert s.as_tuple() == tuple(range(14))


def test_host_properties_come_from_the_integers():
    import kmeans_gpu_amd as kg
    s = kg.ErrorStats.from_array(np.array([100, 50, 0, 400, 900, 1600, 10, 20, 30, 7, 8, 9, 4096 * 100 * 9, 4096 * 25], np.uint64))
    assert s.mse == (4.0, 9.0, 16.0)
    assert s.psnr == pytest.approx(10.0 * np.log10(65025.0 / (29.0 / 3.0)))
    assert s.delta_e_rms == pytest.approx(3.0) and s.delta_e_max == pytest.approx(5.0)
    zero = kg.ErrorStats.from_array(np.array([5] + [0] * 13, np.uint64))
    assert zero.psnr == float("inf") and zero.delta_e_rms == 0.0 and zero.mse == (0.0, 0.0, 0.0)


def _refused(rc, text):
    import kmeans_gpu_amd as kg
    assert rc == -1, rc
    msg = kg.lib().kmg_last_error().decode()
    assert text in msg, msg


def test_argument_refusals_need_no_device():
    import kmeans_gpu_amd as kg
    L = kg.lib()
    pal = np.zeros((3072, 4), np.uint8)
    pp = C.c_void_p(pal.ctypes.data)
    stats = kg.ErrorStats()
    # kmg_dev_compare: what, cutoff, the limits of the index formats -- all before the processor is looked at (it is NULL here)
    dev = lambda fmt, palette, k, cutoff, what: L.kmg_dev_compare(None, None, None, 16, fmt, palette, k, cutoff, what, None, None)
    _refused(dev(0, None, 0, 0, 0), "what = 0")
    _refused(dev(0, None, 0, 0, 4), "what = 4")
    _refused(dev(0, None, 0, 0, 7), "what = 7")
    _refused(dev(0, None, 0, 256, 3), "above 255")
    _refused(dev(3, None, 0, 0, 3), "unknown output format")
    _refused(dev(-1, None, 0, 0, 3), "unknown output format")
    _refused(dev(1, pp, 257, 0, 1), "INDEX8")
    _refused(dev(1, pp, 256, 1, 1), "transparent slot")
    _refused(dev(1, None, 4, 0, 1), "needs a palette")
    _refused(dev(2, pp, 0, 0, 1), "needs a palette")
    _refused(dev(2, pp, 3073, 0, 1), "needs a palette")
    # accepted limits get past these checks and stop at the missing processor
    for args in ((1, pp, 256, 0, 1), (1, pp, 255, 255, 2), (2, pp, 3072, 9, 3), (0, None, 0, 255, 3)):
        _refused(dev(*args), "bad compare arguments")
    # kmg_compare
    cmp_ = lambda fmt, palette, k, what: L.kmg_compare(None, None, None, 4, 4, fmt, palette, k, what, C.byref(stats))
    _refused(cmp_(0, None, 0, 0), "what = 0")
    _refused(cmp_(0, None, 0, 8), "what = 8")
    _refused(cmp_(5, None, 0, 1), "unknown output format")
    _refused(cmp_(1, pp, 257, 1), "INDEX8")
    _refused(cmp_(2, None, 5, 1), "needs a palette")
    _refused(cmp_(0, None, 0, 3), "processor is NULL")
    # kmg_reduce_quality
    rq = lambda k_min, k_max, mode, fmt: L.kmg_reduce_quality(None, None, 4, 4, k_min, k_max, 100, mode, fmt, None, None, None, None, None)
    _refused(rq(0, 8, 0, 0), "colour counts [0, 8]")
    _refused(rq(9, 8, 0, 0), "colour counts [9, 8]")
    _refused(rq(1, 3073, 0, 0), "colour counts [1, 3073]")
    _refused(rq(2, 8, 4, 0), "unknown mode")
    _refused(rq(2, 8, 0, 3), "unknown output format")
    _refused(rq(2, 8, 2, 1), "meld")
    _refused(rq(2, 257, 0, 1), "INDEX8")
    _refused(rq(2, 8, 2, 0), "processor is NULL")            # meld with RGBA8 is a legal request
    _refused(rq(1, 3072, 3, 2), "processor is NULL")


def test_python_surface():
    import kmeans_gpu_amd as kg
    for name in ("compare", "compare_device", "reduce_quality"):
        assert callable(getattr(kg.ImageProcessor, name)), name
    for name in ("mse", "psnr", "delta_e_rms"):
        assert isinstance(getattr(kg.ErrorStats, name), property), name
    assert "ErrorStats" in kg.__all__
    import inspect
    sig = inspect.signature(kg.ImageProcessor.reduce_quality)
    assert list(sig.parameters)[1:] == ["image", "max_delta_e", "k_min", "k_max", "reduce_mode", "indexed"]
    assert (sig.parameters["k_min"].default, sig.parameters["k_max"].default, sig.parameters["indexed"].default) == (2, 256, False)


def _cli_error(argv, capsys):
    from kmeans_gpu_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_cli_flags_and_refusals(capsys, tmp_path):
    from kmeans_gpu_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["reduce", "--help"])
    text = capsys.readouterr().out
    assert "--report" in text and "--max-error" in text and "--min-colors" in text
    with pytest.raises(SystemExit):
        cli.main(["find", "--help"])
    text = capsys.readouterr().out
    assert "--report" in text and "--max-error" not in text
    with pytest.raises(SystemExit):
        cli.main(["palette", "--help"])
    assert "--report" not in capsys.readouterr().out
    img = os.path.join(ROOT, "tests", "golden", "tokyo.png")
    assert "--report is not supported with --devices" in _cli_error(["--devices", "0", "reduce", "-i", img, "-c", "8", "--report"], capsys)
    assert "--report is not supported with --devices" in _cli_error(["--devices", "0,1", "find", "-i", img, "-p", "#000000,#ffffff", "--report"],
                                                                    capsys)
    assert "--max-error is not supported with --devices" in _cli_error(["--devices", "0", "reduce", "-i", img, "-c", "8", "--max-error", "2.5"],
                                                                       capsys)
    assert "octree" in _cli_error(["reduce", "-i", img, "-c", "8", "-a", "octree", "--max-error", "2.5"], capsys)
    assert "--min-colors 9 is above -c 8" in _cli_error(["reduce", "-i", img, "-c", "8", "--max-error", "2", "--min-colors", "9"], capsys)
    assert "--min-colors belongs to --max-error" in _cli_error(["reduce", "-i", img, "-c", "8", "--min-colors", "3"], capsys)
    assert "not a number" in _cli_error(["reduce", "-i", img, "-c", "8", "--max-error", "x"], capsys)
    # the line itself, from a record
    import kmeans_gpu_amd as kg
    s = kg.ErrorStats.from_array(np.array([100, 50, 0, 400, 900, 1600, 10, 20, 30, 7, 8, 9, 4096 * 100 * 9, 4096 * 25], np.uint64))
    assert cli.report_line(s) == "Error: pixels=100 mse=(4.000,9.000,16.000) psnr=38.28dB dE76 rms=3.000 max=5.000"
    assert cli.report_line(s, chosen=12, reached=True).endswith(" colors=12 target reached")
    assert cli.report_line(s, chosen=64, reached=False).endswith(" colors=64 target not reached")
