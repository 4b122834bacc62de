"""What ``support.inference.denoise_frame`` and ``denoise_sample_frame`` hand back, for both model families: the layout of the return
tuple under ``want_pbuffers`` / ``preview``, that neither option changes the frame, and what ``times`` receives.

The values themselves are held by tests/test_gpu_denoise.py and tests/test_gpu_denoise_sample.py, whose stand-in interfaces and
frames are used here.  80 x 72 at 2 spp: two spans per axis, the last origin clamped, four tiles -- at ``batch_size=3`` one full batch
and a ragged one."""
import itertools

import pytest
import torch

import test_gpu_denoise as K
import test_gpu_denoise_sample as S

pytestmark = pytest.mark.gpu

H, W, SPP = 80, 72, 2
OPTIONS = list(itertools.product((False, True), (False, True)))          # (want_pbuffers, preview)


class _SampleTileModel(S._TileIndex):
    """``_TileIndex`` with a P-buffer: the first three path descriptors of the tile."""

    def denoise_batch(self, batch):
        return super().denoise_batch(batch)[0], batch["paths"][:, :, 0:3] * 2.0


class _DictTileModel(K._TileModel):
    """``_TileModel`` with its P-buffers as the dict of two tensors that ``KPCNInterface`` returns."""

    def denoise_batch(self, batch):
        out, p = super().denoise_batch(batch)
        return out, {"diffuse": p, "specular": batch["paths"][:, :, 3:5] * 0.5}


def _kpcn(model, **kw):
    from wcmc_amd.support.inference import denoise_frame
    _, (kpcn, llpm), _ = K._frame(H, W, SPP)
    return denoise_frame(model(), kpcn, llpm, True, batch_size=3, **kw)


def _sample(model, **kw):
    from wcmc_amd.support.inference import denoise_sample_frame
    _, (ss, sp, ll), _ = S._frame(H, W, SPP)
    return denoise_sample_frame(model(), ss, sp, ll, True, True, True, batch_size=3, **kw)


FAMILIES = {"kpcn": (_kpcn, K._TileModel), "sample": (_sample, _SampleTileModel)}


def _check_frame(res):
    out, ipt, has_hit = res[:3]
    for t, shape in ((out, (H, W, 3)), (ipt, (H, W, 3)), (has_hit, (H, W))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == torch.device(K.DEV)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_return_tuple_and_times(family):
    from wcmc_amd.support.inference import frame_tiles
    run, model = FAMILIES[family]
    tiles = len(frame_tiles(H, W))
    assert tiles == 4
    first = None
    for want_pbuffers, preview in OPTIONS:
        times = {}
        res = run(model, want_pbuffers=want_pbuffers, preview=preview, times=times)
        assert isinstance(res, tuple) and len(res) == 3 + int(want_pbuffers) + 2 * int(preview)
        _check_frame(res)
        if want_pbuffers:
            out_path = res[3]
            assert tuple(out_path.shape) == (SPP, 3, H, W) and out_path.dtype == torch.float32
        if preview:
            for pv in res[-2:]:
                assert tuple(pv.shape) == (H, W, 3) and pv.dtype == torch.uint8
        if first is None:
            first = res[:3]
        for a, b in zip(res[:3], first):
            assert torch.equal(a, b)
        assert set(times) == {"network", "finish", "tiles"} and times["tiles"] == tiles
        assert times["network"] > 0 and times["finish"] > 0
    assert len(run(model)) == 3                                   # (the defaults: neither option, no times)


def test_dict_pbuffers_come_back_as_a_dict_with_the_same_keys():
    _, (kpcn, llpm), _ = K._frame(H, W, SPP)
    res = _kpcn(_DictTileModel, want_pbuffers=True)
    assert len(res) == 4
    _check_frame(res)
    out_path = res[3]
    assert isinstance(out_path, dict) and set(out_path) == {"diffuse", "specular"}
    assert tuple(out_path["diffuse"].shape) == (SPP, 3, H, W) and tuple(out_path["specular"].shape) == (SPP, 2, H, W)
    assert torch.equal(out_path["diffuse"], (llpm[..., 1:4] * 2.0).permute(2, 3, 0, 1))
    assert torch.equal(out_path["specular"], (llpm[..., 4:6] * 0.5).permute(2, 3, 0, 1))
    for a, b in zip(res[:3], _kpcn(K._TileModel)):
        assert torch.equal(a, b)
    assert len(_kpcn(_DictTileModel)) == 3
