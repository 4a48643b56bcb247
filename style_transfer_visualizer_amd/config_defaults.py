"""User-facing defaults (values follow reference config_defaults.py:5-41)."""
from __future__ import annotations

# optimisation
DEFAULT_STEPS = 1500
DEFAULT_STYLE_WEIGHT = 1e5
DEFAULT_CONTENT_WEIGHT = 1.0
DEFAULT_TV_WEIGHT = 0.0      # build-specific: weight of the total-variation regulariser (0 = off)
DEFAULT_PYRAMID_LEVELS = 1   # build-specific: levels of a coarse-to-fine run (1 = the single-size run)
DEFAULT_PYRAMID_STEPS = None  # build-specific: steps per level, coarsest first (None = optimization.steps split evenly)
DEFAULT_PRESERVE_COLOR = "off"  # build-specific: keep the content image's colours ("match": style statistics, "luma": chroma swap)
DEFAULT_CONTENT_SIZE = 0     # build-specific: longer side the content image is resized to before the run (0 = keep its size)
DEFAULT_STYLE_SIZE = 0       # build-specific: longer side the style image is resized to (0 = keep its size)
DEFAULT_STYLE_SCALE = 0.0    # build-specific: the style's longer side as a multiple of the content's (0 = keep its size)
DEFAULT_RESIZE_FILTER = "lanczos"  # build-specific: "bilinear" | "bicubic" | "lanczos", antialiased on a downscale
DEFAULT_STYLE_BLEND = None   # build-specific: one blend weight per style image, --style's first (None = equal weights)
DEFAULT_STYLE_LAYER_WEIGHTS = None  # build-specific: one weight per entry of style_layers (None = every layer counts 1)
DEFAULT_LAP_WEIGHT = 0.0     # build-specific: weight of the Laplacian loss against the content image (0 = off)
DEFAULT_LAP_POOLS = [4]      # build-specific: its pool sizes (powers of two from 1 to 32, one to four of them)
DEFAULT_MASK_REGIONS = 2     # build-specific: regions of --content-mask / --style-mask, 2 to 4 uniform grey bands
DEFAULT_REGION_WEIGHTS = None  # build-specific: one weight per region (None = every region counts 1; 0 = left unstyled)
DEFAULT_AUTO_MASK = False    # build-specific: segment the two images into mask_regions colour regions instead of reading masks
DEFAULT_AUTO_MASK_CELL = 8   # build-specific: cell size of that segmentation in pixels (1, 2, 4, 8, 16 or 32)
DEFAULT_AUTO_MASK_SPACE = "color"  # build-specific: where that segmentation clusters, "color" (box means) or "features" (one VGG layer)
DEFAULT_AUTO_MASK_LAYER = 10       # build-specific: the VGG index whose output is clustered in "features" space (conv3_1)
DEFAULT_POOLING = "max"      # build-specific: pooling layers of the feature stack, "max" (VGG as trained) or "avg" (the mean)
DEFAULT_LEARNING_RATE = 1.0
DEFAULT_INIT_METHOD = "random"
DEFAULT_SEED = 0
DEFAULT_NORMALIZE = True
DEFAULT_LBFGS_MAX_ITER = 1
DEFAULT_LBFGS_MAX_EVAL = 1
# indices into vgg19().features: conv1_1, conv2_1, conv3_1, conv4_1, conv5_1 / conv4_2
DEFAULT_STYLE_LAYERS: tuple[int, ...] = (0, 5, 10, 19, 28)
DEFAULT_CONTENT_LAYERS: tuple[int, ...] = (21,)

# video
DEFAULT_SAVE_EVERY = 20
DEFAULT_FPS = 10
DEFAULT_VIDEO_QUALITY = 10
DEFAULT_CREATE_VIDEO = True
DEFAULT_FINAL_ONLY = False
DEFAULT_VIDEO_INTRO_ENABLED = True
DEFAULT_VIDEO_INTRO_DURATION = 10.0
DEFAULT_VIDEO_OUTRO_DURATION = 10.0
DEFAULT_VIDEO_FINAL_FRAME_COMPARE = True
DEFAULT_VIDEO_MODE = "realtime"
DEFAULT_CREATE_GIF = False
DEFAULT_GIF_INCLUDE_INTRO = False
DEFAULT_GIF_INCLUDE_OUTRO = False
DEFAULT_GIF_COLORS = 256       # build-specific: entries of the timelapse GIF's one palette (2..256)
DEFAULT_VIDEO_FORMAT = "mp4"   # build-specific: "mp4" (the reference's container; no encoder in this build) or "mjpeg" (built in)
DEFAULT_GIF_DITHER = "ordered" # build-specific: "ordered" (8x8 Bayer) or "none"

# hardware
DEFAULT_DEVICE = "cuda"
DEFAULT_PRECISION = "fp32"   # build-specific: "bf16" selects bf16 activation storage

# output
DEFAULT_LOG_EVERY = 10
DEFAULT_OUTPUT_DIR = "out"
DEFAULT_SAVE_MASKS = False   # build-specific: write the two label maps of a guided run as grey PNGs into the output directory
