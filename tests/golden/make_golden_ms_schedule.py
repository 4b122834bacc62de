#!/usr/bin/env python3
"""Generate ``tests/golden/ms_schedule.npz`` by driving the REAL reference's ``MSDenoiseDataset`` (support/datasets.py:1149-1171).

Run on the development machine only (the reference tree is not on the GPU machine), as ``make_golden_dataset.py``:

    python tests/golden/make_golden_ms_schedule.py

A three-scene training directory (empty gt files: the constructor only lists them), spp 4, batch size 8.  For every dataset index
``i`` the file records what ``MSDenoiseDataset[i]`` would read without reading it: ``ConcatDataset``'s own index arithmetic
(``cumulative_sizes`` and ``bisect_right``, as its ``__getitem__``) picks the member dataset and the index inside it; the member's
``spp`` is the sample count (:618, :1091), and ``idx // patches_per_image`` the image (:1036).
  counts (n,)  images (n,)  patches_per_image ()  n_images ()  spp ()
"""
import bisect
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

NAMES = ("bathroom.npy", "kitchen.npy", "veach.npy")
SPP, BATCH = 4, 8


def main():
    mg.import_reference()
    np.bool = bool                                     # the reference predates numpy 1.24
    import support.datasets as rd
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "train", "gt"))
        for n in NAMES:
            open(os.path.join(tmp, "train", "gt", n), "wb").close()
        walk = os.walk
        os.walk = lambda d: iter([(d, [], sorted(NAMES))])
        try:
            ms = rd.MSDenoiseDataset(tmp, SPP, base_model="kpcn", mode="train", batch_size=BATCH)
        finally:
            os.walk = walk
        counts, images = [], []
        for i in range(len(ms)):
            d = bisect.bisect_right(ms.cumulative_sizes, i)            # torch.utils.data.ConcatDataset.__getitem__
            j = i if d == 0 else i - ms.cumulative_sizes[d - 1]
            counts.append(ms.datasets[d].spp)
            images.append(j // ms.datasets[d].patches_per_image)       # datasets.py:1036
        try:
            rd.MSDenoiseDataset(tmp, 1, base_model="kpcn", mode="train", batch_size=BATCH)
            low = ""
        except RuntimeError as exc:
            low = str(exc)
    out = {"counts": np.array(counts, dtype=np.int32), "images": np.array(images, dtype=np.int32),
           "patches_per_image": np.array(ms.datasets[0].patches_per_image), "n_images": np.array(len(NAMES)),
           "spp": np.array(SPP), "too_low_message": np.array(low)}
    np.savez_compressed(os.path.join(HERE, "ms_schedule.npz"), **out)
    print("ms_schedule", {k: v.shape for k, v in out.items()}, repr(low))


if __name__ == "__main__":
    main()
