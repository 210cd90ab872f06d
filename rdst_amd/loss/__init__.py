from .seg_unet import SegUNet_F  # noqa: F401
from .sr_loss import LazyScalars, RecLoss, SRLoss  # noqa: F401
from .ssim import SSIMLoss, ssim_loss, window_taps  # noqa: F401
from .consistency import LRConsistencyLoss, lr_consistency_loss, lrc_adjoint, lrc_residual  # noqa: F401
from .msssim import MSSSIMLoss, level_weights, ms_ssim_loss  # noqa: F401
