"""Denoising and evaluating with SBMC / LBMC models, the parts that need no GPU: the argument checks of wcmc_assemble_sample_tiles and
wcmc_finish_sample_frame, the new flags of the two commands and their argument errors, and ``SBMCInterface.denoise_batch``."""
import ctypes

import pytest
import torch


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Negative status + a message, before any HIP call (the contract of include/wcmc_hip.h): this runs without a GPU."""
    from wcmc_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)          # `one`: non-null, aligned, never dereferenced by the checks
    tile_keys = ("sbmc_s", "sbmc_p", "llpm", "origins", "B", "H", "W", "S", "P", "pad", "t", "g", "p", "rad", "feat", "paths", "stream")
    tiles = lambda **kw: L.wcmc_assemble_sample_tiles(*[{**dict(   # noqa: E731
        sbmc_s=one, sbmc_p=one, llpm=one, origins=one, B=2, H=70, W=83, S=2, P=128, pad=32, t=0, g=1, p=1, rad=one, feat=one,
        paths=one, stream=null), **kw}[k] for k in tile_keys])
    fin_keys = ("out_rad", "sbmc_s", "llpm", "H", "W", "S", "out", "ipt", "has_hit", "pv_out", "pv_ipt", "stream")
    finish = lambda **kw: L.wcmc_finish_sample_frame(*[{**dict(   # noqa: E731
        out_rad=one, sbmc_s=one, llpm=one, H=70, W=83, S=2, out=one, ipt=one, has_hit=one, pv_out=null, pv_ipt=null, stream=null),
        **kw}[k] for k in fin_keys])
    cases = [(tiles, dict(sbmc_s=null), "null pointer"), (tiles, dict(origins=null), "null pointer"),
             (tiles, dict(rad=null), "null pointer"), (tiles, dict(feat=null), "null pointer"),
             (tiles, dict(sbmc_p=null), "needs sbmc_p"),                  # use_sbmc_buf without its buffer
             (tiles, dict(paths=null), "paths"),                          # llpm without a paths output
             (tiles, dict(S=0), "S must be positive"), (tiles, dict(S=-3), "S must be positive"),
             (tiles, dict(P=64), "no interior"), (tiles, dict(P=63), "no interior"), (tiles, dict(pad=64), "no interior"),
             (tiles, dict(H=32), "pad = 32 must be smaller"), (tiles, dict(H=40, W=40), "does not fit"),
             (tiles, dict(B=0), "positive"), (tiles, dict(pad=-1), "non-negative"), (tiles, dict(t=8), "0..7"),
             (finish, dict(out_rad=null), "null pointer"), (finish, dict(sbmc_s=null), "null pointer"),
             (finish, dict(llpm=null), "null pointer"), (finish, dict(ipt=null), "null pointer"),
             (finish, dict(S=0), "must be positive"), (finish, dict(W=0), "must be positive")]
    for fn, kw, text in cases:
        rc = fn(**kw)
        msg = L.wcmc_last_error().decode()
        assert rc < 0, (kw, rc)
        assert text in msg and ("assemble_sample_tiles" if fn is tiles else "finish_sample_frame") in msg, (kw, msg)


SAMPLE_FLAGS = ["--denoiser", "pkg.mod:make", "--disentangle", "m11r01", "--use_sbmc_buf", "--lr_dncnn", "0.001"]


def test_both_parsers_accept_the_sample_based_flags():
    from wcmc_amd import denoise, evaluate
    a = denoise.build_parser().parse_args(["--input", "a.npy", "--output_dir", "o", "--tile_pad", "16"] + SAMPLE_FLAGS)
    b = evaluate.build_parser().parse_args(["--input_dir", "d"] + SAMPLE_FLAGS)
    for args in (a, b):
        assert (args.denoiser, args.disentangle, args.use_sbmc_buf, args.lr_dncnn, args.use_g_buf) == ("pkg.mod:make", "m11r01", True, 0.001, True)
    assert a.tile_pad == 16 and not hasattr(b, "tile_pad")
    d = denoise.build_parser().parse_args(["--input", "a.npy", "--output_dir", "o"])
    assert (d.tile_pad, d.denoiser, d.use_sbmc_buf, d.use_g_buf) == (32, None, False, True)


def test_a_sample_based_model_without_a_denoiser_is_refused_before_any_file_is_looked_for(tmp_path):
    from wcmc_amd import denoise, evaluate
    from wcmc_amd.train_sbmc import DenoiserFactoryError
    missing = str(tmp_path / "nothing.npy")
    for name in ("SBMC_x", "LBMC_x"):
        argv = ["--input", missing, "--output_dir", "o", "--save", str(tmp_path), "--model_name", name]
        with pytest.raises(DenoiserFactoryError, match="--denoiser"):
            denoise.check_inputs(denoise.build_parser().parse_args(argv))
        with pytest.raises(DenoiserFactoryError, match="--denoiser"):
            denoise.check_inputs(denoise.build_parser().parse_args(argv + ["--denoiser", "no_such_package_xyz.models:make"]))
        with pytest.raises(DenoiserFactoryError, match="--denoiser"):
            evaluate.denoise(evaluate.build_parser().parse_args(["--input_dir", str(tmp_path), "--model_name", name]), str(tmp_path),
                             str(tmp_path / "o"), ["scene"], device="cpu")
    # with a factory that resolves, the next thing looked for is the file
    with pytest.raises(FileNotFoundError):
        denoise.check_inputs(denoise.build_parser().parse_args(
            ["--input", missing, "--output_dir", "o", "--model_name", "SBMC_x", "--denoiser", "standins:SampleDenoiserStandIn"]))
    with pytest.raises(ValueError, match="no interior"):
        denoise.check_inputs(denoise.build_parser().parse_args(
            ["--input", missing, "--output_dir", "o", "--model_name", "SBMC_x", "--denoiser", "standins:SampleDenoiserStandIn",
             "--tile_pad", "64"]))


def test_the_tile_pad_of_a_kpcn_model_is_32(tmp_path):
    from wcmc_amd import denoise
    argv = ["--input", str(tmp_path / "nothing.npy"), "--output_dir", "o", "--model_name", "KPCN_x"]
    with pytest.raises(ValueError, match="--tile_pad 16"):
        denoise.check_inputs(denoise.build_parser().parse_args(argv + ["--tile_pad", "16"]))
    with pytest.raises(FileNotFoundError):                        # 32 is accepted: the next check is the input file
        denoise.check_inputs(denoise.build_parser().parse_args(argv + ["--tile_pad", "32"]))


class _MeanOfSamples(torch.nn.Module):
    """An identity-like stand-in denoiser: the mean radiance over the samples."""

    def forward(self, data):
        assert set(data) == {"radiance", "features"}
        return data["radiance"].mean(1)


@pytest.mark.parametrize("cls", ["SBMCInterface", "LBMCInterface"])
def test_denoise_batch_needs_no_target_and_scores_nothing(cls):
    from wcmc_amd.support import interfaces
    lf = {"l_recon": torch.nn.L1Loss(), "l_test": torch.nn.L1Loss()}
    itf = getattr(interfaces, cls)({"dncnn": _MeanOfSamples()}, {}, lf, None)
    itf.to_eval_mode()
    itf.m_losses["m_val"] = torch.tensor(0.5)
    before = {k: v.clone() for k, v in itf.m_losses.items()}
    batch = {"radiance": torch.rand(2, 3, 3, 8, 8), "features": torch.rand(2, 3, 5, 8, 8)}
    out, p_buffer = itf.denoise_batch(batch)
    assert p_buffer is None and torch.equal(out, batch["radiance"].mean(1))
    assert set(batch) == {"radiance", "features"}                 # the caller's dictionary is left as it was
    assert set(itf.m_losses) == set(before) and all(torch.equal(itf.m_losses[k], before[k]) for k in before)
    with pytest.raises(KeyError, match="target_image"):           # validate_batch is the route that scores, and it needs the target
        itf.validate_batch(dict(batch))
