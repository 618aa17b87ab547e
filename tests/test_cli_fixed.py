"""`--fixed` of the command line (kmeans_gpu_amd/cli.py): the palette files `reduce --indexed` and `sequence` write start with the
pinned colours' bytes, in the order given; `palette` contains them; the refusals of the argument parser."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXED = "#000000,#FFFFFF,#C81E1E"
BYTES = [0, 0, 0, 255, 255, 255, 200, 30, 30]


def _frames(tmp_path, n):
    from PIL import Image
    rng = np.random.default_rng(77)
    paths = []
    for i in range(n):
        img = rng.integers(0, 256, (37, 61, 4), dtype=np.uint8)
        img[..., 3] = 255
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(img, "RGBA").save(paths[-1])
    return paths


def test_reduce_fixed(torch_cuda, tmp_path, capsys):
    from PIL import Image
    from kmeans_gpu_amd import cli
    src = _frames(tmp_path, 1)[0]
    out = str(tmp_path / "out.png")
    assert cli.main(["reduce", "-i", src, "-c", "7", "--indexed", "--fixed", FIXED, "-o", out]) == 0
    img = Image.open(out)
    assert img.mode == "P" and img.getpalette()[:9] == BYTES
    # RGBA output: only palette colours, and without --fixed another result
    rgba, plain = str(tmp_path / "rgba.png"), str(tmp_path / "plain.png")
    assert cli.main(["reduce", "-i", src, "-c", "7", "--fixed", FIXED, "-o", rgba]) == 0
    assert cli.main(["reduce", "-i", src, "-c", "7", "-o", plain]) == 0
    a, b = np.array(Image.open(rgba).convert("RGBA")), np.array(Image.open(plain).convert("RGBA"))
    assert np.array_equal(a[..., :3], np.array(img.convert("RGB"))) and not np.array_equal(a, b)
    # palette: the pins are among its (sorted) colours
    pal = str(tmp_path / "pal.png")
    capsys.readouterr()
    assert cli.main(["palette", "-i", src, "-c", "7", "--fixed", FIXED, "-o", pal, "-s", "1"]) == 0
    line = capsys.readouterr().out
    for c in FIXED.split(","):
        assert c in line
    for bad in (["reduce", "-i", src, "-c", "2", "--fixed", FIXED], ["reduce", "-i", src, "-c", "7", "-a", "octree", "--fixed", FIXED],
                ["--devices", "0", "reduce", "-i", src, "-c", "7", "--fixed", FIXED], ["reduce", "-i", src, "-c", "7", "--fixed", "red"],
                ["reduce", "-i", src, "-c", "7", "--max-error", "3", "--min-colors", "2", "--fixed", FIXED]):
        with pytest.raises(SystemExit):
            cli.main(bad)


def test_sequence_fixed(torch_cuda, tmp_path):
    from PIL import Image
    from kmeans_gpu_amd import cli
    paths = _frames(tmp_path, 3)
    out = str(tmp_path / "seq.png")
    assert cli.main(["sequence", "-i", *paths, "-c", "6", "--fixed", FIXED, "-o", out]) == 0
    img = Image.open(out)
    assert img.mode == "P" and img.getpalette()[:9] == BYTES
    with pytest.raises(SystemExit):
        cli.main(["sequence", "-i", *paths, "-c", "2", "--fixed", FIXED, "-o", out])
