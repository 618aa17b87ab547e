"""Alpha mode (kmg_options.alpha_cutoff) on every route of the output pass, bit for bit against tests/alpha_ref.py.

With a forced strategy the route follows from (strategy, k, mode) alone: a `forced` of -1 or +1 (`forced_strategy` of the
processor) short-circuits every `*_pays` cost model of csrc/kmg_apply_route.h (except `diffuse_table_pays`, which answers false for
k < 2 before it looks at `forced`), and `dither_takes_lists` is `!mask_words && k <= kRouteListMaxK (512)` with `mask_words` =
`strategy & KMG_STRATEGY_MASK_WORDS`.  From `apply_route`:

    dither         = mode == DITHER && k > 1
    meld           : k >= 2 && meld_pruning_pays                          -> kMeldLists if dither_takes_lists, else kMeldMasks
    colour table   : DIFFUSE ? diffuse_table_pays : !dither && replace_table_pays          -> kDiffuseTable / kReplaceTable
    pruned dither  : dither && dither_pruning_pays                        -> kDitherLists if dither_takes_lists, else kDitherMasks
    otherwise        kMeldScan (meld), kDiffuseScan (diffuse), kScan: the default k_apply route (replace, dither)

and from `run_band` / `run_diffuse` of csrc/kmg_apply.hip and the launchers: k_apply is chunked for k >= 32; the label tables are u8 for k <= 256,
u16 above, and kReplaceTable / kDitherMasks are followed by k_alpha_merge in alpha mode; the Lab lists have two halves for k > 256;
kDitherMasks launches k_dither_sorted for one mask word (k <= 64), else k_dither_pruned<W> with W = 1, 2, 4 words or 0 (any other
count); kDiffuseTable runs kDiffusePairs for k <= 256 and kDiffuseCells above.

| strategy           | k                 | replace (0)                   | dither (1)                                 | meld (2)          | diffuse (3)     |
|--------------------|-------------------|-------------------------------|--------------------------------------------|-------------------|-----------------|
| `scan`             | 5 / 40            | k_apply unchunked / chunked   | same, DITHER                               | k_meld scan       | kDiffuseScan    |
| `table`            | 1                 | label table u8 + merge        | same as replace (k = 1 is never dither)    | scan (needs k>=2) | kDiffuseScan    |
| `table`            | 24                | label table u8 + merge        | lists, 1 half                              | lists, 1 half     | kDiffusePairs   |
| `table`            | 300               | label table u16 + merge       | lists, 2 halves                            | lists, 2 halves   | kDiffuseCells   |
| `table`            | 600               | label table u16 + merge       | masks, W = 0 + merge                       | masks             | kDiffuseCells   |
| `table+mask_words` | 40 / 100 / 150 / 200 | (as `table`)               | k_dither_sorted / W = 2 / W = 0 / W = 4 + merge | masks        | (as `table`)    |

(k = 1 under `table` diffuses through the scan: `diffuse_table_pays` refuses k < 2 whatever the strategy.)

Every (strategy, k, mode) runs on one 1001 x 300 image -- half blobs, half uniform noise, random alpha weighted towards 0, t - 1, t
and 255 -- through kmg_dev_apply on the whole image and through one apply plan in three bands on two streams.  The bands start at
rows 0, 1 and 167: with the odd width the second and third start 1001 and 167167 pixels in, so their input and output pointers are
not 16-byte aligned (the `aligned == 0` paths of the kernels and of k_alpha_merge).  Modes 0-2 pass alpha through only, so t = 1
and t = 255 give the same bytes; diffusion runs at t = 1, 128 and 255.  The same processor at alpha_cutoff 0 gives the default
call's bytes (the kernels' non-ALPHA instantiations on the same input)."""
import numpy as np
import pytest

import alpha_ref
import diffuse_ref
from conftest import set_strategy

pytestmark = pytest.mark.gpu

W, H = 1001, 300
BANDS = [0, 1, 167, H]
CUTOFFS = (1, 128, 255)

ROUTES = ([("scan", k, m) for k in (5, 40) for m in (0, 1, 2, 3)] +
          [("table", k, m) for k in (1, 24, 300, 600) for m in (0, 1, 2, 3)] +
          [("table+mask_words", k, m) for k in (40, 100, 150, 200) for m in (1, 2)])


def _image(oracle):
    rng = np.random.default_rng(1001)
    n = W * H
    half = n // 2
    c = rng.integers(0, 256, (25, 3))
    blobs = np.clip(np.rint(c[rng.integers(0, 25, half)] + rng.normal(0, 25.0, (half, 3))), 0, 255).astype(np.uint8)
    img = oracle.synth_uniform(77, n)
    img[:half, :3] = blobs
    special = np.array([0, 0, 1, 127, 128, 254, 255, 255], np.uint8)        # 0, t - 1, t, 255 for t = 1, 128, 255
    a = rng.integers(0, 256, n).astype(np.uint8)
    pick = rng.random(n) < 0.5
    a[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    img[:, 3] = a
    return np.ascontiguousarray(img.reshape(H, W, 4))


@pytest.fixture(scope="module")
def image(oracle):
    return _image(oracle)


@pytest.fixture(scope="module")
def procs(torch_cuda):
    """one processor per cutoff"""
    import kmeans_gpu_amd as kg
    ps = {t: kg.ImageProcessor(alpha_cutoff=t) for t in CUTOFFS}
    yield ps
    for p in ps.values():
        p.close()


_palettes = {}


def _palette(oracle, k):
    if k not in _palettes:
        pal = np.array(sorted(set(map(tuple, oracle.synth_uniform(k + 9, k)))), np.uint8)
        assert pal.shape[0] == k
        _palettes[k] = pal
    return _palettes[k]


def _whole(torch, proc, d_in, cent, mode):
    out = torch.full_like(d_in, 0x5A)
    proc.apply(d_in.data_ptr(), W, H, 0, cent, mode, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(H, W, 4)


def _banded(torch, proc, d_in, cent, mode):
    """one plan, three bands, alternating between two streams"""
    assert BANDS[0] == 0 and BANDS[-1] == H and all(a < b for a, b in zip(BANDS, BANDS[1:]))
    out = torch.full_like(d_in, 0x5A)
    torch.cuda.synchronize()
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    plan = proc.apply_plan(cent, mode, W * H, streams[0].cuda_stream)
    try:
        for i in range(len(BANDS) - 1):
            r0, r1 = BANDS[i], BANDS[i + 1]
            plan.run(d_in.data_ptr() + 4 * r0 * W, W, r1 - r0, r0, out.data_ptr() + 4 * r0 * W, streams[i % 2].cuda_stream)
        torch.cuda.synchronize()
        plan.status()
    finally:
        plan.close()
    return out.cpu().numpy().reshape(H, W, 4)


@pytest.mark.parametrize("strategy,k,mode", ROUTES)
def test_route_in_alpha_mode(oracle, torch_cuda, procs, image, strategy, k, mode):
    import kmeans_gpu_amd as kg
    torch = torch_cuda
    set_strategy(strategy)
    cent = kg.palette_to_centroids(_palette(oracle, k))
    d_in = torch.from_numpy(image.reshape(-1, 4)).cuda()
    if mode == alpha_ref.MODE_DIFFUSE:
        near = diffuse_ref.Nearest(diffuse_ref.oracle_apply_replace(oracle, cent))
        for t in CUTOFFS:
            want = alpha_ref.diffuse(image, None, t, nearest=near)
            assert np.array_equal(_whole(torch, procs[t], d_in, cent, mode), want), f"kmg_dev_apply, t = {t}"
            assert np.array_equal(_banded(torch, procs[t], d_in, cent, mode), want), f"plan in bands, t = {t}"
        default = diffuse_ref.diffuse(image, None, nearest=near)
    else:
        default = oracle.apply(image, cent, mode)
        want = alpha_ref.with_alpha(default, image)
        assert np.array_equal(_whole(torch, procs[1], d_in, cent, mode), want), "kmg_dev_apply, t = 1"
        assert np.array_equal(_banded(torch, procs[1], d_in, cent, mode), want), "plan in bands, t = 1"
        assert np.array_equal(_whole(torch, procs[255], d_in, cent, mode), want), "kmg_dev_apply, t = 255"
    assert (default[..., 3] == 255).all()
    p = procs[1]
    p.set_alpha_cutoff(0)
    try:
        assert np.array_equal(_whole(torch, p, d_in, cent, mode), default), "kmg_dev_apply, alpha_cutoff 0"
        assert np.array_equal(_banded(torch, p, d_in, cent, mode), default), "plan in bands, alpha_cutoff 0"
    finally:
        p.set_alpha_cutoff(1)
