"""What the CPU and the GPU tests of the pipes' colour hand-over share (tests/test_cpu_colour.py: the plan judgement without a
device; tests/test_gpu_colour_pipe.py: the same refusals through the setters)."""
from openjph_amd import pipeline

W, H = 66, 34
C = pipeline.Colour
# (format, colour, container, what the plan is made with): every one refused with E_INVALID
PLAN_REFUSALS = [
    ("v410", "bt709", 16, dict(depth=10)),                                   # Y, Cb, Cr already
    ("y410", "bt709", 16, dict(depth=10)),
    ("ayuv", "bt709", 16, dict(depth=8)),
    ("y4xx", "bt709", 16, dict(depth=12)),
    ("y416", "bt709", 16, dict(depth=16)),
    ("uyvy", "bt709", 16, dict(depth=8, cell=(2, 1))),                       # not of the 4:4:4 family
    ("v210", "bt709", 16, dict(depth=10, cell=(2, 1))),
    ("nv12", "bt709", 16, dict(depth=8, cell=(2, 2))),
    ("r210", "bt709", 16, dict(depth=10, num_comps=4)),                      # not three components
    ("r210", "bt709", 16, dict(depth=10, num_comps=1)),
    ("r210", "bt709", 16, dict(depth=10, signs=[False, True, True])),        # a signed component
    ("r210", "bt709", 16, dict(depth=10, is_signed=True)),
    ("r210", "bt709", 16, dict(depth=10, bit_depths=[10, 8, 8])),            # mixed depths
    ("r210", C("bt709", rgb_depth=10), 32, dict(depth=17)),                  # a depth above 16
    ("r210", C("bt709", rgb_depth=10), 16, dict(depth=7)),                   # ... below 8: no table
    ("r210", "bt709", 16, dict(depth=10, downsampling=[(1, 1), (4, 1), (4, 1)])),   # a factor other than 1 or 2
    ("r210", "bt709", 16, dict(depth=10, downsampling=[(1, 1), (1, 4), (1, 4)])),
    ("r210", "bt709", 16, dict(depth=10, downsampling=[(1, 1), (2, 1), (1, 1)])),   # Cb and Cr sub-sampled differently
    ("r210", "bt709", 16, dict(depth=10, downsampling=[(1, 1), (2, 2), (2, 1)])),
    ("r210", "bt709", 16, dict(depth=10, downsampling=[(2, 1), (2, 1), (2, 1)])),   # luma off the reference grid
    ("bgra", "bt709", 16, dict(depth=10)),                                   # rgb_depth 0 = the plan's 10: not what BGRA holds
    ("bgra", C("bt709", rgb_depth=10), 16, dict(depth=10)),
    ("argb", C("bt709", rgb_depth=9), 16, dict(depth=8)),
    ("r210", C("bt709", rgb_depth=12), 16, dict(depth=12)),
    ("r10k", "bt709", 16, dict(depth=12)),
    ("r210", C("bt709", rgb_depth=7), 16, dict(depth=10)),                   # an RGB depth below 8: no table
    ("r210", "bt709", 8, dict(depth=8)),                                     # a dword format in 8-bit containers
    ("rgba", C("bt709", rgb_depth=8), 8, dict(depth=10)),                    # the plan's depth above the container
    ("r210", "bt709", 16, dict(depth=10, cell=(2, 1), image_offset=(1, 0))), # an odd image offset in a halved direction: phase 1
    ("r210", "bt709", 16, dict(depth=10, cell=(2, 2), image_offset=(0, 1))),
    ("r210", "bt709", 16, dict(depth=10, cell=(2, 2), image_offset=(3, 5))),
]
