"""The image sizes at which whole networks are run off the square, power-of-two path (test_rect_cases_cpu.py holds this
table against the library's own kernel choice; test_gpu_rect_model.py and test_gpu_rect_uresnet.py run the networks).

Every test of a whole network elsewhere in the suite uses a square power-of-two image (64, 128, 256), where all three
transposed convolutions of the generator take the fused four-tap kernels and every 3x3 layer takes Winograd, and where
height and width can be exchanged anywhere in the model code without a test noticing.  These are the smallest sizes that
reach the other branches of the layer tables (model.hip deconv_fused / deconv_wgrad_all, dg_conv_plan):

  fused_fwd / fused_wgrad: the generator's transposed convolutions (DECONVS order) that take deconv_fwd_kernel /
      deconv_wgrad_kernel in an fp32 context; the others take the grouped implicit GEMM and colsum + four per-tap
      weight gradients.
  wino: the critics' 3x3 layers (CRITIC_3X3 order) that take the Winograd kernel in forward and backward-data; the others
      take the direct implicit GEMM, in the same pass.
"""
from collections import namedtuple

DECONVS = ("de_gen_9", "de_gen_11", "de_gen_15")            # at H/8, H/4, H/2 with 128, 96, 64 channels
DECONV_LEVEL = {"de_gen_9": (8, 128), "de_gen_11": (4, 96), "de_gen_15": (2, 64)}
CRITIC_3X3 = ("dis_2", "dis_3", "dis_4", "dis_5", "dis_6", "dis_7", "dis_8")
# (name, channels in, channels out, divisor of the image size) of the critics' 3x3 layers
CRITIC_LEVEL = {"dis_2": (32, 64, 4), "dis_3": (64, 64, 4), "dis_4": (64, 128, 8), "dis_5": (128, 128, 8),
                "dis_6": (128, 256, 16), "dis_7": (256, 256, 16), "dis_8": (256, 256, 16)}

RectCase = namedtuple("RectCase", "name H W B fused_fwd fused_wgrad wino why")

NONE, ALL = (), DECONVS
CASES = [
    RectCase("48x80", 48, 80, 2, NONE, NONE, CRITIC_3X3[:4],
             "no deconv level (6x10, 12x20, 24x40) is a power of two; the critic bottom is 3x5: dis_6/7/8 go direct next to "
             "Winograd layers; every level is a ragged 16x16 tile"),
    RectCase("16x48", 16, 48, 2, NONE, NONE, CRITIC_3X3[:4],
             "the minimum height: generator levels down to 2x6, the critic bottom 1x3 (a 3x3 conv on a one-row image), "
             "a Flatten of 3"),
    RectCase("96x32", 96, 32, 2, NONE, NONE, CRITIC_3X3,
             "H > W; the generator bottom is 12x4 (W = 4 a power of two below the fused forward's minimum of 8, H = 12 none); "
             "the critic bottom 6x2 is even: Winograd on a sub-tile image"),
    RectCase("32x128", 32, 128, 2, ALL, ALL, CRITIC_3X3,
             "powers of two with H != W: the fused deconv kernels at 4x16, 8x32, 16x64 (lgH != lgW) -- the negative control"),
    RectCase("48x80-b3", 48, 80, 3, NONE, NONE, CRITIC_3X3[:4],
             "an odd batch: B*H*W % 32 and the persistent / item thresholds at another item count"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

# refused by depgan_create: a height or a width that is no multiple of 16
REFUSED = [(40, 80), (48, 72)]
# the sizes the DEP-UResNet tests run at (batch 4, n = 4 and a short batch n = 3)
URESNET_SIZES = [(48, 80), (16, 48), (32, 128)]
