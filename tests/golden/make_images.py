"""Writes tests/golden/images.npz: the two images of the reference's image workflows as uint8 arrays, at full size
and at the examples' default rescales (get_image in their utils.py: PIL NEAREST to (int(W r), int(H r)), per channel).

    python tests/golden/make_images.py /path/to/reference

house  examples/image-denoising/img/house.png   (256, 256)     rescale 0.4 -> house_r04
castle examples/image-inpainting/img/castle.jpg (481, 321, 3)  rescale 0.1 -> castle_r01
"""
import os
import sys

import numpy as np
from PIL import Image


def rescaled(img, r):
    target = (int(img.shape[1] * r), int(img.shape[0] * r))
    if img.ndim == 3:
        return np.stack([np.asarray(Image.fromarray(img[:, :, ch]).resize(target, resample=Image.NEAREST))
                         for ch in range(img.shape[2])], axis=2)
    return np.asarray(Image.fromarray(img).resize(target, resample=Image.NEAREST))


def main(ref):
    ex = os.path.join(ref, "examples")
    house = np.asarray(Image.open(os.path.join(ex, "image-denoising", "img", "house.png")), dtype=np.uint8)
    castle = np.asarray(Image.open(os.path.join(ex, "image-inpainting", "img", "castle.jpg")), dtype=np.uint8)
    out = {"house": house, "house_r04": rescaled(house, 0.4), "castle": castle, "castle_r01": rescaled(castle, 0.1)}
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "images.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
