"""The reference's ``train_lbmc.py`` on this build's loop: ``LBMCInterface`` around a base denoiser the caller supplies.

As ``wcmc_amd.train_sbmc`` (which holds what the two share); model construction and losses follow ``train_lbmc.py:67-204``: the
dataset is 'lbmc' (the g-buffer without the SBMC buffers), the reconstruction loss is ``SMAPE`` of both images clamped to
[0, 100], and the denoiser's Adam is stepped down by ``StepLR(step_size=3, gamma=0.5)`` (:196-198).  ``--denoiser
package.module:factory`` stands where the reference imports layerdenoise's ``LayerNet(n_in, tonemap, True)``.

    python -m wcmc_amd.train_lbmc --from_data_dir --data_dir D --denoiser my_pkg.models:make_layernet --desc ... --use_llpm_buf \
        --manif_learn --manif_loss FMSE
"""
import argparse
import itertools
import os

import torch

from . import train_sbmc as ts
from .support.interfaces import LBMCInterface
from .support.losses import SMAPE, RelativeMSE


class ClampedSMAPE(torch.nn.Module):
    """``recon_loss`` of ``train_lbmc.py:164-165``."""

    def __init__(self):
        super().__init__()
        self.smape = SMAPE()

    def forward(self, im, ref):
        return self.smape(torch.clamp(im, min=0, max=1e2), torch.clamp(ref, min=0, max=1e2))


def init_data(args, device):
    return ts.init_data(args, device, base_model='lbmc', use_sbmc_buf=False)


def init_model(sizes, args, device):
    """``train_lbmc.py:67-204``."""
    interfaces, params = [], {}
    grid = list(itertools.product(args.lr_pnet, args.pnet_out_size, args.w_manif))
    for lr_pnet, pnet_out_size, w_manif in grid:
        print('Train a LBMC network.')
        models = ts.build_models(sizes, args, pnet_out_size, args.use_llpm_buf, 'LBMC')
        model_fn = ts.model_file(args, grid, lr_pnet, pnet_out_size, w_manif)
        optims, ck = ts.restore_and_optimizers(models, args, model_fn, lr_pnet, device)
        loss_funcs = ts.tk.with_dssim(args, ts.manifold_loss(args, {'l_recon': ClampedSMAPE(), 'l_test': RelativeMSE()}), ('l_recon',))
        itf = LBMCInterface(models, optims, loss_funcs, args, args.use_llpm_buf, args.manif_learn, w_manif, args.disentangle)
        if ck is not None and args.best_err is not None:
            print('Use the checkpoint best error %.3e' % (args.best_err))
            itf.best_err = args.best_err
        interfaces.append(itf)
    params['plots'] = {}
    params['data_device'] = device
    # Required for LBMC (train_lbmc.py:195-198)
    params['sched_dncnn'] = torch.optim.lr_scheduler.StepLR(optims['optim_dncnn'], step_size=3, gamma=0.5,
                                                            last_epoch=args.start_epoch - 1)
    if ck is not None and 'sched_dncnn' in ck.get('params', {}):
        params['sched_dncnn'].load_state_dict(ck['params']['sched_dncnn'].state_dict())
    os.makedirs(args.save, exist_ok=True)
    return interfaces, params


def build_parser():
    return ts.add_common_arguments(argparse.ArgumentParser(description=__doc__.split('\n')[0], epilog=ts.tk.MULTI_SPP_EPILOG), use_sbmc_buf=False)


def main(argv=None):
    args = ts.check_args(ts.tk.parse_args(argv, build_parser()))
    return ts.run(args, init_data, init_model)


if __name__ == '__main__':
    main()
