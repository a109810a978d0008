"""Drop-in for the reference's ``extract_radiomics.py``: reads the frames at ``config['dir']['df']`` / ``['df_test']``,
extracts the radiomic features of every lesion on the device and pickles one frame per split to
``config['dir']['radiomics']`` / ``['radiomics_test']`` -- the frames ``DermDataset(df, radiomics)`` takes.

The reference runs PyRadiomics on the whole decoded image and mask of every record, once per channel, in a process pool
(``RadiomicExtractor.py``).  Here the images are decoded whole (``DermDataset(..., crop=False)``), uploaded in chunks of at most
``--max-bytes`` as ``ImagePool``s and handed to ``isic_hip.radiomics.radiomics_frame`` (one launch per chunk): the
first-order, GLCM and GLDM classes of ``params.yml`` on the original image type, 224 columns named as the reference names
them (``original_<class>_<Feature>_<gs|red|green|blue>``).  The other classes and the filtered image types are not built.

    python extract_radiomics.py --config_path config.yml
    python extract_radiomics.py --synthetic 64 --out radiomics_synthetic.pkl
"""
import argparse

import pandas as pd
import torch
import yaml


def extract(dataset, device, max_bytes=1 << 30, bin_width=10, label=255):
    """-> a frame with one row per item of ``dataset`` (the ``DermDataset`` dict contract with uint8 arrays), its pools
    never above ``max_bytes`` (3 + 1 bytes per pixel)."""
    from isic_hip.augment import ImagePool
    from isic_hip.radiomics import feature_names, radiomics_frame
    frames, items, staged = [], [], 0

    def flush():
        nonlocal staged
        if items:
            frames.append(radiomics_frame(ImagePool.from_arrays(items, device), bin_width=bin_width, label=label))
            items.clear()
            staged = 0

    for i in range(len(dataset)):
        item = dataset[i]
        img, mask = item["image"], item.get("mask")
        need = 4 * int(img.shape[0]) * int(img.shape[1])
        if need > max_bytes:
            raise ValueError(f"image {i} needs {need} bytes: above max_bytes={max_bytes}")
        if staged + need > max_bytes:
            flush()
        items.append((img, mask))
        staged += need
    flush()
    if not frames:
        return pd.DataFrame(columns=feature_names(), dtype="float64")
    return pd.concat(frames, axis=0, ignore_index=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_path", type=str, default="config.yml", help="path to the .yml config file (dir.df, dir.radiomics, ...)")
    ap.add_argument("--max-bytes", type=int, default=1 << 30, help="device bytes of one image pool (4 per pixel)")
    ap.add_argument("--bin-width", type=int, default=10, help="params.yml: binWidth")
    ap.add_argument("--label", type=int, default=255, help="params.yml: label")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="run on N SyntheticDermPixels images, no files read")
    ap.add_argument("--out", type=str, default=None, help="with --synthetic: where to pickle the frame")
    ap.add_argument("--device", type=str, default=None)
    args, _ = ap.parse_known_args(argv)
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic:
        from isic_hip.augment import SyntheticDermPixels
        device = torch.device(args.device or "cuda:0")
        frame = extract(SyntheticDermPixels(args.synthetic), device, args.max_bytes, args.bin_width, args.label)
        print(f"{len(frame)} synthetic images, {frame.shape[1]} features, {int(frame.isna().all(axis=1).sum())} without a mask")
        if args.out:
            frame.to_pickle(args.out)
            print(f"saved {args.out}")
        return frame
    from dataset import DermDataset
    from isic_hip.augment import uint8_transform
    with open(args.config_path) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    device = torch.device(args.device or config.get("device", "cuda:0"))
    for src, dst in (("df", "radiomics"), ("df_test", "radiomics_test")):
        df = pd.read_pickle(config["dir"][src])
        frame = extract(DermDataset(df, None, transform=uint8_transform, crop=False), device, args.max_bytes, args.bin_width,
                        args.label)
        frame.to_pickle(config["dir"][dst])
        print(f"{src}: {len(frame)} records -> {config['dir'][dst]}")


if __name__ == "__main__":
    main()
