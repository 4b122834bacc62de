"""Offline preprocessing of a dataset directory on the GPU: the counterpart of the reference's
``DenoiseDataset._offline_preprocess`` (``support/datasets.py:584-715``) for the KPCN base model.

    python -m wcmc_amd.preprocess --data_dir D --mode train|val|test --spp S [--overwrite] [--no_llpm] [--sbmc] [--device_id N]

Reads ``D/<mode>/input/<scene>.npy`` (H, W, S, 104) and ``D/<mode>/gt/<scene>.npy`` (H, W, 9) and writes, next to the input,
``<scene>_kpcn_<s>.npy``, ``<scene>_llpm.npy`` (+ ``_llpm_<k>.npy`` per continuation file ``<scene>_<k>.npy``), the sanitised gt
and -- outside the test mode -- ``<scene>_prob_imp.npy`` (``support.datasets.DenoiseDirectory.offline_preprocess``).  These are
the files ``wcmc_amd.train_kpcn --from_data_dir`` and ``wcmc_amd.evaluate`` read.  ``--sbmc`` adds ``<scene>_sbmc_s.npy`` / ``_sbmc_p.npy``
(+ ``_sbmc_s_<k>.npy`` / ``_sbmc_p_<k>.npy`` per continuation file): what ``support.datasets.SampleFullImageDataset`` reads.  One line
per scene: files written, seconds.
"""
import argparse
import os

import torch

from .support.datasets import DenoiseDirectory


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--data_dir', type=str, required=True, help='dataset root: <data_dir>/<mode>/{gt,input}/<scene>.npy')
    p.add_argument('--mode', type=str, required=True, choices=('train', 'val', 'test'))
    p.add_argument('--spp', type=int, required=True, help='samples per pixel read from each input file')
    p.add_argument('--overwrite', action='store_true', help='rewrite files that exist')
    p.add_argument('--no_llpm', action='store_true', help='do not write the _llpm files')
    p.add_argument('--sbmc', action='store_true', help='also write the _sbmc_s / _sbmc_p files of the sample-based models')
    p.add_argument('--patch_size', type=int, default=DenoiseDirectory.PATCH_SIZE, help='patch size of the probability map')
    p.add_argument('--device_id', type=int, default=0)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    device = torch.device('cuda', args.device_id)
    torch.cuda.set_device(device)
    d = DenoiseDirectory(args.data_dir, args.spp, args.mode, device=device, patch_size=args.patch_size)
    report = lambda e: print('%s: %d files written (%s), %.2f s' % (                                # noqa: E731
        e[0], len(e[1]), ' '.join(os.path.basename(f) for f in e[1]) or '-', e[2]), flush=True)
    return d.offline_preprocess(llpm=not args.no_llpm, kpcn=True, overwrite=args.overwrite, report=report, sbmc=args.sbmc)


if __name__ == '__main__':
    main()
