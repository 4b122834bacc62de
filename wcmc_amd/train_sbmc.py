"""The reference's ``train_sbmc.py`` on this build's loop: ``SBMCInterface`` around a base denoiser the caller supplies.

``train_kpcn.train`` (epochs, ``latest_<name>.pth``, validation with checkpoint-on-best), the checkpoint helpers and the
``--from_data_dir`` data path are shared with ``wcmc_amd.train_kpcn``; model construction and losses follow ``train_sbmc.py:63-184``:
one ``PathNet`` backbone, ``n_in`` by ``--disentangle``, ``TonemappedRelativeMSE`` + ``RelativeMSE`` (+ FMSE / GRS), Adam.

What differs, on purpose:

  * the base denoiser -- ``sbmc.Multisteps`` in the reference, an import from outside its tree -- stays an external import:
    ``--denoiser package.module:factory`` names a callable, called as ``factory(n_in)`` (``n_in``: the per-sample feature channels the
    interface hands over), that returns an ``nn.Module`` mapping the batch dictionary (``radiance`` (B, S, 3, h, w), ``features``
    (B, S, n_in, h, w)) to a (B, 3, h', w') image.  No stand-in ships in the package;
  * data comes from ``--from_data_dir`` only (``support.datasets.DenoiseDirectory(base_model='sbmc')`` through
    ``support.loader.PatchLoader``: the SBMC buffers are computed on the device from the staged raw frame), at the one sample
    count ``--num_samples`` or, with ``--multi_spp``, at every count 2..``--num_samples`` as the reference's ``MSDenoiseDataset``
    does (``train_sbmc.py:41-44``; the flags and the order: ``wcmc_amd.train_kpcn``);
  * one process, one GPU; no visdom.

    python -m wcmc_amd.train_sbmc --from_data_dir --data_dir D --denoiser my_pkg.models:make_multisteps --desc ... --use_sbmc_buf
"""
import argparse
import importlib
import itertools
import os

import torch

from . import train_kpcn as tk
from .support import checkpoint as ckpt
from .support.interfaces import SBMCInterface
from .support.losses import FeatureMSE, GlobalRelativeSimilarityLoss, RelativeMSE, TonemappedRelativeMSE
from .support.networks import PathNet

BS_VAL = 4          # validation batch size (train_sbmc.py:233)


class DenoiserFactoryError(RuntimeError):
    """``--denoiser`` is missing, cannot be imported, or did not return an ``nn.Module``."""


def load_denoiser_factory(spec):
    """``package.module:factory`` -> the callable.  Every failure is a ``DenoiserFactoryError`` that quotes the flag."""
    if not spec:
        raise DenoiserFactoryError("--denoiser package.module:factory is required: the base denoiser (sbmc.Multisteps / "
                                   "layerdenoise's LayerNet in the reference) is not part of this package")
    mod, sep, attr = spec.partition(':')
    if not sep or not mod or not attr:
        raise DenoiserFactoryError("--denoiser '%s': expected package.module:factory" % spec)
    try:
        module = importlib.import_module(mod)
    except ImportError as exc:
        raise DenoiserFactoryError("--denoiser '%s': cannot import module '%s' (%s)" % (spec, mod, exc)) from exc
    factory = getattr(module, attr, None)
    if not callable(factory):
        raise DenoiserFactoryError("--denoiser '%s': module '%s' has no callable '%s'" % (spec, mod, attr))
    return factory


def make_denoiser(args, n_in):
    model = load_denoiser_factory(getattr(args, 'denoiser', None))(n_in)
    if not isinstance(model, torch.nn.Module):
        raise DenoiserFactoryError("--denoiser '%s': factory(%d) returned %s, not an nn.Module" % (args.denoiser, n_in, type(model).__name__))
    return model


# ------------------------------------------------------------------------------------------------- data
def init_data(args, device, base_model='sbmc', use_sbmc_buf=None):
    """``train_sbmc.py:38-60`` over a dataset directory: use_g_buf=True and pnet_out_size=0, as there."""
    from .support.datasets import DenoiseDirectory
    from .support.loader import PatchLoader
    if not getattr(args, 'from_data_dir', False):
        raise RuntimeError('the sample-based launchers read a dataset directory: pass --from_data_dir --data_dir <dir>')
    use_sbmc_buf = getattr(args, 'use_sbmc_buf', False) if use_sbmc_buf is None else use_sbmc_buf
    kw = dict(use_llpm_buf=args.use_llpm_buf, device=device, patch_size=args.patch_size, pnet_out_size=0, base_model=base_model,
              use_g_buf=True, use_sbmc_buf=use_sbmc_buf)
    tr = DenoiseDirectory(args.data_dir, args.num_samples, 'train', args.batch_size, 'random', **kw)
    va = DenoiseDirectory(args.data_dir, args.num_samples, 'val', BS_VAL, 'grid', **kw)
    ms, counts = tk.multi_spp_loader_args(args)
    train = PatchLoader(tr.reader, range(len(tr)), device, batch_size=args.batch_size, patch_size=args.patch_size,
                        use_llpm=args.use_llpm_buf, patches_per_image=args.patches_per_image, staged_hook=tr.staged_hook,
                        base_model=tr.base_model, use_g_buf=tr.use_g_buf, use_sbmc_buf=tr.use_sbmc_buf, **ms,
                        **tk.augment_loader_args(args))
    val = tk.GridValLoader(va, range(len(va)), BS_VAL, counts=counts)
    sizes = {'dncnn_in_size': tr.dncnn_in_size, 'pnet_in_size': tr.pnet_in_size, 'pnet_out_size': tr.pnet_out_size}
    return sizes, {'train': train, 'val': val}


# ------------------------------------------------------------------------------------------------- models
def model_file(args, grid, lr_pnet, pnet_out_size, w_manif):
    if len(grid) == 1:
        return os.path.join(args.save, args.model_name + '.pth')
    return os.path.join(args.save, '%s_lp%f_pos%d_wgt%f.pth' % (args.model_name, lr_pnet, pnet_out_size, w_manif))


def build_models(sizes, args, pnet_out_size, with_backbone, what):
    """The denoiser and, with the path descriptors, the one PathNet backbone (train_sbmc.py:75-86, train_lbmc.py:79-94)."""
    models = {}
    if with_backbone:
        half = args.disentangle in ('m10r01', 'm11r01')
        n_in = sizes['dncnn_in_size'] + (pnet_out_size // 2 if half else pnet_out_size)
        models['dncnn'] = make_denoiser(args, n_in)
        print('Initialize the %s for path descriptors (# of input channels: %d).' % (what, n_in))
        print('Train a LLPM feature extractor. (# of input channels: %d, # of output channels: %d).'
              % (sizes['pnet_in_size'], pnet_out_size))
        models['backbone'] = PathNet(ic=sizes['pnet_in_size'], outc=pnet_out_size)
    else:
        n_in = sizes['dncnn_in_size']
        models['dncnn'] = make_denoiser(args, n_in)
        print('Initialize the %s for vanilla buffers (# of input channels: %d).' % (what, n_in))
    return models


def restore_and_optimizers(models, args, model_fn, lr_pnet, device):
    """Weights from ``model_fn`` when ``--start_epoch`` is not 0, the models on ``device``, one Adam per model with the stored
    state (train_sbmc.py:98-162).  Returns (optims, checkpoint or None)."""
    assert args.start_epoch != 0 or not os.path.isfile(model_fn), 'Model %s already exists.' % (model_fn)
    ck = ckpt.load_checkpoint(model_fn) if args.start_epoch != 0 and os.path.isfile(model_fn) else None
    if ck is not None:
        ckpt.precision_note(ck)
        ckpt.restore_models(ck, models)
        print('Pretraining weights are loaded.')
    else:
        print('Train models from scratch.')
    for name in models:
        models[name] = models[name].to(device)
    lrs = {'optim_' + name: (args.lr_dncnn if name == 'dncnn' else lr_pnet) for name in models}
    optims = {key: torch.optim.Adam(models[key[len('optim_'):]].parameters(), lr=lr) for key, lr in lrs.items()}
    if ck is not None:
        ckpt.restore_optims(ck, optims, lrs, lr_ckpt=args.lr_ckpt)
    return optims, ck


def manifold_loss(args, loss_funcs):
    if args.manif_learn:
        if args.manif_loss == 'FMSE':
            loss_funcs['l_manif'] = FeatureMSE()
            print('Manifold loss: FeatureMSE')
        elif args.manif_loss == 'GRS':
            loss_funcs['l_manif'] = GlobalRelativeSimilarityLoss()
            print('Manifold loss: Global Relative Similarity')
    else:
        print('Manifold loss: None (i.e., ablation study)')
    return loss_funcs


def init_model(sizes, args, device):
    """``train_sbmc.py:63-200``."""
    interfaces = []
    grid = list(itertools.product(args.lr_pnet, args.pnet_out_size, args.w_manif))
    for lr_pnet, pnet_out_size, w_manif in grid:
        print('Train a SBMC network.')
        if args.use_llpm_buf and not args.use_sbmc_buf:
            models = build_models(sizes, args, pnet_out_size, True, 'SBMC')
        elif args.use_sbmc_buf or (args.use_g_buf and not args.manif_learn):
            models = build_models(sizes, args, pnet_out_size, False, 'SBMC')
        else:
            raise RuntimeError('No such feature combination defined.')
        model_fn = model_file(args, grid, lr_pnet, pnet_out_size, w_manif)
        optims, ck = restore_and_optimizers(models, args, model_fn, lr_pnet, device)
        loss_funcs = tk.with_dssim(args, manifold_loss(args, {'l_recon': TonemappedRelativeMSE(), 'l_test': RelativeMSE()}), ('l_recon',))
        itf = SBMCInterface(models, optims, loss_funcs, args, args.visual, args.use_llpm_buf, args.manif_learn, w_manif,
                            args.use_sbmc_buf, args.disentangle)
        if ck is not None and args.best_err is not None:
            print('Use the checkpoint best error %.3e' % (args.best_err))
            itf.best_err = args.best_err
        interfaces.append(itf)
    os.makedirs(args.save, exist_ok=True)
    return interfaces, {'plots': {}, 'data_device': device}


# ------------------------------------------------------------------------------------------------- command line
def add_common_arguments(p, use_sbmc_buf):
    """support/utils.py:69-100 (BasicArgumentParser) + train_sbmc.py:235-271 / train_lbmc.py:235-269, then this build's."""
    p.add_argument('--sbmc', action='store_true')
    p.add_argument('--p_buf', action='store_true')
    p.add_argument('--model_name', type=str, default='tSUNet', help='name of the model.')
    p.add_argument('--data_dir', type=str, default='./data', help='directory of dataset: <data_dir>/{train,val}/{gt,input}/<scene>.npy')
    p.add_argument('--visual', action='store_true', help='accepted for compatibility; there is no visdom here')
    p.add_argument('-b', '--batch_size', type=int, default=64, help='batch size.')
    p.add_argument('-e', '--num_epoch', type=int, default=100, help='number of epochs.')
    p.add_argument('-v', '--val_epoch', type=int, default=1, help='validate the model every val_epoch epoch.')
    p.add_argument('--vis_iter', type=int, default=4)
    p.add_argument('--start_epoch', type=int, default=0, help='from which epoch to start.')
    p.add_argument('--num_samples', type=int, default=8)
    p.add_argument('--save', type=str, default='./weights', help='directory to save the model.')
    p.add_argument('--overfit', action='store_true')
    p.add_argument('--desc', type=str, required=True, help='short description of the current experiment.')
    p.add_argument('--single_gpu', action='store_true', help='accepted for compatibility (one process drives one GPU)')
    p.add_argument('--device_id', type=int, default=0, help='device id')
    p.add_argument('--lr_ckpt', action='store_true', help='keep the learning rate stored in the checkpoint.')
    p.add_argument('--best_err', type=float, required=False)
    p.add_argument('--use_g_buf', action='store_false')
    p.add_argument('--lr_dncnn', type=float, default=1e-4, help='learning rate of the base denoiser.')
    if use_sbmc_buf:
        p.add_argument('--use_sbmc_buf', action='store_true', help='use the sbmc-specific buffer.')
    p.add_argument('--use_llpm_buf', action='store_true', help='use the llpm-specific buffer.')
    p.add_argument('--manif_learn', action='store_true', help='use the manifold learning loss.')
    p.add_argument('--pnet_out_size', type=int, nargs='+', default=[3], help='# of channels of outputs of PathNet.')
    p.add_argument('--lr_pnet', type=float, nargs='+', default=[0.0001], help='learning rate of PathNet.')
    p.add_argument('--manif_loss', type=str, required=False, help='`FMSE` or `GRS`')
    p.add_argument('--w_manif', type=float, nargs='+', default=[0.1],
                   help='ratio of the manifold learning loss to the reconstruction loss.')
    p.add_argument('--disentangle', type=str, default='m11r11', help='`m11r11`, `m10r01`, `m10r11`, or `m11r01`')
    p.add_argument('--not_save', action='store_true', help='do not save checkpoint (debugging purpose).')
    # this build
    p.add_argument('--denoiser', type=str, default=None, metavar='package.module:factory',
                   help='the base denoiser: factory(n_in) -> nn.Module mapping the batch dictionary to (B, 3, h, w).  Required')
    p.add_argument('--from_data_dir', action='store_true',
                   help='train on <data_dir>/train and validate on <data_dir>/val at --num_samples samples per pixel')
    p.add_argument('--patch_size', type=int, default=128)
    p.add_argument('--patches_per_image', type=int, default=None,
                   help='patches drawn per image and epoch (default: (256 // batch_size) * batch_size)')
    return p


def build_parser():
    return add_common_arguments(argparse.ArgumentParser(description=__doc__.split('\n')[0], epilog=tk.MULTI_SPP_EPILOG), use_sbmc_buf=True)


def check_args(args):
    """The argument errors of ``train_sbmc.py:275-287`` (those of ``train_kpcn.py``), and the factory: it is resolved before any
    file is read."""
    tk.check_args(args)
    load_denoiser_factory(args.denoiser)
    return args


def run(args, init_data_fn, init_model_fn):
    import numpy as np
    device = torch.device('cuda', args.device_id)
    torch.cuda.set_device(device)
    np.random.seed(0)                                                  # train_sbmc.py:205-207
    torch.manual_seed(0)
    sizes, dataloaders = init_data_fn(args, device)
    interfaces, params = init_model_fn(sizes, args, device)
    params['rank'] = 0
    tk.train(interfaces, dataloaders, params, args)
    return interfaces


def main(argv=None):
    args = check_args(tk.parse_args(argv, build_parser()))
    return run(args, init_data, init_model)


if __name__ == '__main__':
    main()
