"""Evaluate a trained KPCN, SBMC or LBMC model on full scenes: the counterpart of the reference's ``test_models.denoise``
(``test_models.py:104-277``).

For every scene x spp: ``support.datasets.FullImageDataset`` (tiles assembled on the GPU from the offline-preprocessed files),
``support.inference.stitched_inference`` (the network + one stitch launch per batch), the valid crop, and
``support.metrics.evaluate_frame`` on the cropped frames (the has-hit composite inside the kernel): the 5 metrics (RelMSE, RelL1,
DSSIM, L1, MSE) under 4 tone maps (linear, _tonemap, tonemap, tonemap28) for the output and for the noisy input.
``results[(5*t + k)*len(spps) + j][i]`` is written to ``results_<model_name>_<spps[-1]>.csv`` and
``results_input_<spps[-1]>.csv`` as the reference does.

    python -m wcmc_amd.evaluate --save WEIGHTS_DIR --model_name KPCN_manifold --input_dir DATA/test/input \\
        --output_dir OUT --scenes bathroom car --spps 8 32 [--use_llpm_buf --manif_learn --manif_loss FMSE ...]

The model flags are those of ``wcmc_amd.train_kpcn``; the model is ``<save>/<model_name>.pth`` (a ``train_kpcn``
checkpoint) loaded through ``train_kpcn.init_model``.  A model whose name holds ``SBMC`` / ``LBMC`` is a ``train_sbmc`` /
``train_lbmc`` checkpoint around the caller's base denoiser (``--denoiser package.module:factory``, required; ``--use_sbmc_buf``,
``--disentangle`` as those launchers define them): its tiles come from ``support.datasets.SampleFullImageDataset`` (the offline
``_sbmc_s`` / ``_sbmc_p`` files), its interface from that launcher's ``init_model``, and everything after the network is the same.
The reference's quantize / TensorRT branches and its commented-out PFM output are not carried over.
"""
import os

import numpy as np
import torch

from . import train_kpcn
from .support import metrics as M
from .denoise import _model_path, add_sample_arguments, restore_interface, sample_launcher
from .support.datasets import FullImageDataset, SampleFullImageDataset
from .support.inference import stitched_inference

VALID_SIZE = 72                     # test_models.py:217-218
PATCH_SIZE = 128


def load_input(filename, spp, args, device=None):
    """test_models.py:37-46."""
    if 'KPCN' in args.model_name:
        return FullImageDataset(filename, spp, 'kpcn', args.use_g_buf, args.use_sbmc_buf, args.use_llpm_buf,
                                args.pnet_out_size[0], device=device)
    assert 'BMC' in args.model_name, args.model_name
    return SampleFullImageDataset(filename, spp, 'sbmc', args.use_g_buf, args.use_sbmc_buf, args.use_llpm_buf, 0, device=device)


def denoise(args, input_dir, output_dir="../test_suite_2", scenes=None, spps=(8,), save_figures=False, rhf=False,
            device=None, frames=None):
    """test_models.denoise.  Returns ``(results, results_input)`` as (20 * len(spps), len(scenes)) arrays (None after
    ``rhf``).  ``frames``: an optional dict that receives ``frames[(scene, spp)] = (out, ipt, tgt)``, the cropped (H, W, 3)
    device frames the metrics were taken of (``out`` after the has-hit composite)."""
    assert os.path.isdir(input_dir), input_dir
    assert 'KPCN' in args.model_name or 'BMC' in args.model_name, args.model_name
    if 'KPCN' not in args.model_name:
        assert sample_launcher(args.model_name) is not None, args.model_name
        from .train_sbmc import load_denoiser_factory
        load_denoiser_factory(getattr(args, 'denoiser', None))        # (a DenoiserFactoryError, before any file is looked for)
    device = torch.device(device if device is not None else torch.cuda.current_device())
    spps = list(spps)
    if scenes is None:
        scenes = sorted(fn for fn in os.listdir(input_dir.replace(os.sep + 'input', os.sep + 'gt')) if fn.endswith(".npy"))
    num_metrics = 5 * 4
    results = np.zeros((num_metrics * len(spps), len(scenes)))
    results_input = np.zeros((num_metrics * len(spps), len(scenes)))

    p_model = _model_path(args)
    if not os.path.isfile(p_model):
        raise FileNotFoundError(p_model)
    print(scenes)
    for scene in scenes:
        if not scene.endswith(".npy"):
            scene = scene + '.npy'
        filename = os.path.join(input_dir, scene).replace(os.sep + 'input', os.sep + 'gt')
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)

    crop = (PATCH_SIZE - VALID_SIZE) // 2
    interface = None
    for i, scene in enumerate(scenes):
        if scene.endswith(".npy"):
            scene = scene[:-4]
        print("Scene file: ", scene)
        os.makedirs(os.path.join(output_dir, scene), exist_ok=True)
        for j, spp in enumerate(spps):
            print("Samples per pixel:", spp)
            dataset = load_input(os.path.join(input_dir, scene + ".npy"), spp, args, device)
            if interface is None:                  # (after the first dataset has loaded; KPCN-Ref is evaluated too)
                interface = restore_interface(args, device)           # test_models.py:163-171
            out_rad, out_path = stitched_inference(interface, dataset, PATCH_SIZE, args.use_llpm_buf)

            if out_path is not None and rhf:
                print('Saving P-buffer as numpy file for RHF-like visualization...')
                p = out_path['diffuse'] if isinstance(out_path, dict) else out_path
                p = p.permute(2, 3, 0, 1).cpu().numpy()
                print('Shape: ', p.shape)
                np.save(os.path.join(output_dir, 'p_buffer_%s_%s.npy' % (scene, args.model_name)), p)
                print('Saved.')
                return None

            # valid crop (views of the frames; the kernel takes strides) and the has-hit composite inside the kernel
            out_v = out_rad.permute(1, 2, 0)[crop:-crop, crop:-crop]
            tgt = dataset.full_tgt[crop:-crop, crop:-crop]
            ipt = dataset.full_ipt[crop:-crop, crop:-crop]
            has_hit = dataset.has_hit[crop:-crop, crop:-crop]
            row_out, row_ipt = M.evaluate_frame(out_v, ipt, tgt, has_hit)
            print(row_out[5 * 2 + 0])              # RelMSE(tonemap(out_rad), tonemap(tgt))   test_models.py:250
            print(row_ipt[5 * 2 + 0])              # RelMSE(tonemap(ipt), tonemap(tgt))       test_models.py:251
            for t in range(4):
                for k in range(5):
                    results[(5 * t + k) * len(spps) + j][i] = row_out[5 * t + k]
                    results_input[(5 * t + k) * len(spps) + j][i] = row_ipt[5 * t + k]

            if frames is not None or save_figures:
                out_c = torch.where(has_hit == 0, ipt, out_v)
                if frames is not None:
                    frames[(scene, spp)] = (out_c, ipt, tgt)
                if save_figures:
                    _save_figures(os.path.join(output_dir, scene), spp, args.model_name, out_c, ipt, tgt)

    np.savetxt(os.path.join(output_dir, 'results_{}_{}.csv'.format(args.model_name, spps[-1])), results, delimiter=',')
    np.savetxt(os.path.join(output_dir, 'results_input_%d.csv' % (spps[-1])), results_input, delimiter=',')
    return results, results_input


def _save_figures(d, spp, model_name, out, ipt, tgt):
    """test_models.py:256-270: the four PNGs (tonemap28 of target / input / output, the RelMSE error map in magma)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    tm = lambda x: M.tonemap(x, kInvGamma=1 / 2.8).cpu().numpy()          # noqa: E731
    err = ((out - tgt) ** 2 / (tgt ** 2 + M.EPS))                           # RelMSE(out, tgt, reduce=False), unraveled
    t_err = torch.clamp(err ** 0.45, 0.0, 1.0).mean(2).cpu().numpy()
    plt.imsave(os.path.join(d, 'target.png'), tm(tgt))
    plt.imsave(os.path.join(d, 'input_{}.png'.format(spp)), tm(ipt))
    plt.imsave(os.path.join(d, 'output_{}_{}.png'.format(spp, model_name)), tm(out))
    plt.imsave(os.path.join(d, 'errmap_rmse_{}_{}.png'.format(spp, model_name)), t_err, cmap=plt.get_cmap('magma'))


def build_parser():
    p = train_kpcn.build_parser()
    p.description = "Evaluate a trained KPCN, SBMC or LBMC model on full scenes (test_models.denoise)."
    for a in p._actions:
        if a.dest == 'desc':
            a.required = False                     # a training-run label; not needed to evaluate
    p.add_argument('--input_dir', type=str, required=True, help='directory of the <scene>.npy inputs (a path with /input/)')
    p.add_argument('--output_dir', type=str, default='../test_suite_2', help='where the CSVs and figures go')
    p.add_argument('--scenes', type=str, nargs='*', default=None, help='scene names (default: every .npy under gt/)')
    p.add_argument('--spps', type=int, nargs='+', default=[8])
    p.add_argument('--save_figures', action='store_true', help='write the four PNGs per scene and spp (needs matplotlib)')
    p.add_argument('--rhf', action='store_true', help="save the P-buffer of the first scene (KPCN: the diffuse one) as .npy and stop")
    return add_sample_arguments(p)


def main(argv=None):
    args = train_kpcn.check_args(build_parser().parse_args(argv))
    device = torch.device('cuda', args.device_id)
    torch.cuda.set_device(device)
    input_dir = args.input_dir if args.input_dir.endswith(os.sep) else args.input_dir + os.sep
    denoise(args, input_dir, args.output_dir, args.scenes, args.spps, args.save_figures, args.rhf, device)


if __name__ == '__main__':
    main()
