"""python -m meta_interpolation_amd.main --model sepconv --synthetic ...   (reference: main.py:1-11)

Under torch.distributed.run (one process per GPU) the meta-batch is sharded across ranks with one
RCCL all-reduce of outer gradients per iteration; with a single process it is the sequential loop.

--model dain adapts its tasks one by one in the eager loop unless --dain_task_modes 1 is given: then --task_batch, --graph_inner_loop and
--task_streams mean for it what they mean for the other plugins (config.py; not with --second_order, not on the host).

--model adacof (an addition: the reference has no such plugin) is the SepConv U-Net with AdaCoF's deformable-tap tail on fused HIP kernels
(adacof/model.py; --adacof_kernel_size, --adacof_dilation); every task mode of the SepConv plugin applies, --second_order and the host take
the op composed from torch ops.

--model softsplat (another addition) forward-warps both frames to the time stamp with softmax splatting on fused HIP kernels
(softsplat/model.py; --softsplat_alpha, --softsplat_mode) between Super SloMo's flow U-Net and a refinement U-Net; a
pretrained_models/softsplat_base.pth is loaded as adacof_base.pth is (no public checkpoint was on hand: not verified); every task mode
applies, --second_order takes the op composed from torch ops and needs --warp_second_order 1 for the metric's backward warp."""
from .config import get_args
from .data import MetaLearningSystemDataLoader
from .experiment_builder import ExperimentBuilder
from .meta_learning_system import SceneAdaptiveInterpolation
from . import task_parallel


def main(argv=None):
    args, _ = get_args(argv)
    if args.cuda:
        task_parallel.init_from_env()
    print(args)
    model = SceneAdaptiveInterpolation(args)
    data = MetaLearningSystemDataLoader
    savfi_system = ExperimentBuilder(model=model, data=data, args=args)
    return savfi_system.run_experiment()


if __name__ == '__main__':
    main()
