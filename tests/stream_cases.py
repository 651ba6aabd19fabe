"""The frame-preparation cases shared by test_stream_ref.py (CPU: what the
restatement says about them) and test_stream_gpu.py (the kernel against it).
Each is the smallest shape that reaches its branch: sizes that are no multiple
of 16, more than one workgroup of 256 threads x 4 pixels, border taps."""

# barrel, 8 numbers (EuRoC's coefficients at a small focal length): 50 x 84 crops to 48 x 80,
# the map stays inside the source
BARREL = dict(shape=(50, 84), calib=(40, 41, 41.3, 24.6, -0.2834, 0.0739, 1.9e-4, 1.76e-5))
# 9 numbers: the map reaches -0.94 and 95.49, so border taps are partly outside
NINE = dict(shape=(64, 96), calib=(60, 58, 47.7, 31.2, 0.07, -0.08, 1e-3, -2e-3, 0.01))
# pincushion: the corners read far outside the source, all four taps
PINCUSHION = dict(shape=(50, 84), calib=(40, 41, 41.3, 24.6, 0.3, 0.0, 0.0, 0.0))
# 4 numbers: the pure crop path
PLAIN = dict(shape=(50, 84), calib=(40, 41, 41.3, 24.6))

# a pixel is left out of the bit comparison only where the floor of the map is within this of
# flipping (a last-bit difference between host and device arithmetic), and at most this share
MARGIN = 1e-6
MAX_EXCLUDED = 1e-3
