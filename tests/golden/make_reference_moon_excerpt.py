#!/usr/bin/env python
"""Generates tests/golden/reference_moon_excerpt.npz: frames 20000-25999 (both channels, int16) of the reference's own sample data,
datasets/moon/audio/003.0000.wav, and the file's sample rate.  Data only: 24 KB of samples the reference ships, which the
resampling tests (tests/test_resample_gpu.py) take at the rate, width and channel count the reference's data really has.

`python tests/golden/make_reference_moon_excerpt.py <reference checkout>`.  Run once by hand where a reference checkout exists;
never by a test."""
import os
import sys

import numpy as np
from scipy.io import wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, LAST = 20000, 26000


def main(ref):
    rate, data = wavfile.read(os.path.join(ref, "datasets", "moon", "audio", "003.0000.wav"))
    assert data.dtype == np.int16 and data.ndim == 2 and data.shape[1] == 2 and len(data) >= LAST, (data.dtype, data.shape)
    dst = os.path.join(HERE, "reference_moon_excerpt.npz")
    np.savez_compressed(dst, frames=np.ascontiguousarray(data[FIRST:LAST]), sample_rate=np.int64(rate), first_frame=np.int64(FIRST))
    print("wrote", dst, os.path.getsize(dst), "bytes; rate", rate, "peak", int(np.abs(data[FIRST:LAST]).max()))


if __name__ == "__main__":
    main(sys.argv[1])
