"""Lesion flags per patch, read from the patch-level frames of ``save_latent.extract_latents``: what ``05_train_gnns.py
--lesion-flags`` trains on and ``04_measure_heterophily.py --lesion-flags`` measures (the subgraph the flags induce)."""
import os
import pickle
from pathlib import Path

import numpy as np
import pandas as pd


def _frame(path):
    with Path(path).open("rb") as fh:
        obj = pickle.load(fh)
    return obj if isinstance(obj, pd.DataFrame) else pd.DataFrame(obj)


def load_lesion_flags(paths):
    """-> {image id: (patch ids [m], flags [m])} from patch-level frames as ``save_latent.extract_latents`` returns them
    (columns ``image_path`` or ``image_id``, ``patch_id``, ``patch_in_mask``): the patches of one image in patch-id order,
    the way `01_train_mil_teacher.py` forms its bags.  The image id is the ``image_id`` column, else the file name of
    ``image_path`` without its extension."""
    flags = {}
    for path in paths:
        df = _frame(path)
        missing = {"patch_id", "patch_in_mask"} - set(df.columns)
        if missing or not ({"image_id", "image_path"} & set(df.columns)):
            raise ValueError(f"{path}: not a patch-level frame (needs image_path or image_id, patch_id, patch_in_mask)")
        ids = df["image_id"].astype(str) if "image_id" in df.columns else \
            df["image_path"].map(lambda p: os.path.splitext(os.path.basename(str(p)))[0])
        for image_id, grp in df.assign(_image=ids.values).groupby("_image", sort=False):
            grp = grp.sort_values("patch_id")
            flags[str(image_id)] = (grp["patch_id"].to_numpy(dtype=np.int64), grp["patch_in_mask"].to_numpy() != 0)
    return flags


def _keep_flags(lesion_flags, image_id, n):
    """The ``keep`` array [n] of one record: the image's flags in patch order when the frame has all n patches, else placed
    at their patch ids (a frame written with ``remove_background=True`` lists the lesion patches only)."""
    if image_id not in lesion_flags:
        raise ValueError(f"No lesion flags for image {image_id}")
    pid, flag = lesion_flags[image_id]
    if len(pid) == n:
        return flag.copy()
    if len(pid) > n or (len(pid) and (pid.min() < 0 or pid.max() >= n)) or len(np.unique(pid)) != len(pid):
        raise ValueError(f"Lesion flags of image {image_id} do not fit its {n} patches")
    keep = np.zeros(n, dtype=bool)
    keep[pid] = flag
    return keep
