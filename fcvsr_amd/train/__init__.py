"""Training half of the hot path (SURVEY section 8 rows b-callers, e-train, f2): a differentiable forward whose convolutions
(98 % of the FLOPs) run on the HIP kernels in both directions, the Charbonnier losses of the reference and its focal frequency loss
(`focal_frequency_loss`, `charbonnier_ffl_loss`: one half-spectrum transform of the difference, fixed-order sums), and a data-parallel
step with a flat-buffer gradient all-reduce over RCCL.  `DeviceClipSampler` cuts the training batches on the device from resident
uint8 or uint16 (10-bit) sequences.  `fit_iters` is the iteration loop with
resumable checkpoints: `HipAdam` (the whole update in one launch, the state two flat buffers), stateless schedules, atomic writes."""
from .ops import conv2d                      # noqa: F401
from .graph import forward_train             # noqa: F401
from .loss import (charbonnier_ffl_loss, charbonnier_loss, charbonnier_loss_mmedit, ffl_reference,   # noqa: F401
                   focal_frequency_loss)
from .step import FlatGradAllReduce, TrainStep, fit_iters, iter_position   # noqa: F401
from .optim import HipAdam, adam_step_host                    # noqa: F401
from .schedule import cosine_restart_lr, multistep_lr, schedule_lr       # noqa: F401
from .checkpoint import latest, load_checkpoint, save_checkpoint         # noqa: F401
from .data import BatchPlan, DeviceClipSampler, apply_plan_host          # noqa: F401
