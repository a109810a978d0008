"""Drop-in for the helpers of the reference's ``utils.py`` that compute or parse: ``get_args_parser`` (reference
`utils.py:151-158`), which the MIL / GNN path uses, and ``concat_patch_moments`` (`utils.py:16-31`), the per-image
descriptor of the MAE path's latent space, here one HIP launch (``isic_hip.moments.token_moments``).  The UMAP /
reconstruction visualisers of that file are reporting code outside the path."""
import argparse
import os
import typing


def concat_patch_moments(latent, eps=1e-6, unbiased=False, keep=None):
    """latent [B, T, D] fp32 on the device -> [B, 6 D]: mean, max, std, median, skewness, excess kurtosis over the
    tokens, the reference's concatenation order.  ``keep`` [B, T] (non-zero keeps the token) restricts image b to its kept
    tokens (a NaN row where none is kept).  No backward; no CPU fallback."""
    from isic_hip.moments import token_moments
    return token_moments(latent, eps=eps, unbiased=unbiased, keep=keep)


def get_args_parser(path: typing.Union[str, bytes, os.PathLike]):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config_path", type=str, default=path,
                        help="path to the .yml config file specifying datasets / training params")
    return parser
