"""`python -m moge_amd.scripts.cli eval_baseline` - the reference's benchmark harness (moge/scripts/eval_baseline.py) on the MI355X path: the
data warp of moge_amd.evaluation, the model behind any `Baseline` plugin file (e.g. baselines/moge_mi355x.py) and moge_amd.metrics.

Same options (`--baseline`, `--config`, `--output/-o`, `--oracle`, `--dump_pred`, `--dump_gt`); every other argument goes to the plugin's
click command `Baseline.load`.  Same timing of `inference_time` (synchronise, timer around the call, synchronise inside the timer) and the
same results file: one `key_average` per benchmark, rewritten every 100 samples and after the last one, and a final `mean` entry.  Dumps
use moge_amd.io's EXR / colour-map writers and PIL; the dump layout is the reference's."""
import json
import time
from pathlib import Path

import click


@click.command(context_settings={"allow_extra_args": True, "ignore_unknown_options": True}, help="Evaluation script.")
@click.option("--baseline", "baseline_code_path", type=click.Path(), required=True, help="Path to the baseline model python code.")
@click.option("--config", "config_path", type=click.Path(), default="configs/eval/all_benchmarks.json", help="Path to the evaluation configurations. "
              'Defaults to "configs/eval/all_benchmarks.json".')
@click.option("--output", "-o", "output_path", type=click.Path(), required=True, help="Path to the output json file.")
@click.option("--oracle", "oracle_mode", is_flag=True, help="Use oracle mode for evaluation, i.e., use the GT intrinsics input.")
@click.option("--dump_pred", is_flag=True, help="Dump predition results.")
@click.option("--dump_gt", is_flag=True, help="Dump ground truth.")
@click.pass_context
def main(ctx: click.Context, baseline_code_path: str, config_path: str, oracle_mode: bool, output_path: str, dump_pred: bool, dump_gt: bool):
    import torch

    from moge_amd.evaluation import EvalDataLoader, key_average
    from moge_amd.metrics import compute_metrics
    from moge_amd.scripts.infer_baseline import import_file_as_module

    module = import_file_as_module(baseline_code_path, Path(baseline_code_path).stem)
    baseline = getattr(module, "Baseline").load.main(ctx.args, standalone_mode=False)

    with open(config_path, "r") as f:
        config = json.load(f)

    Path(output_path).parent.mkdir(parents=True, exist_ok=True)
    all_metrics = {}
    for benchmark_name, benchmark_config in config.items():
        metrics_list = []
        with EvalDataLoader(**benchmark_config, device=baseline.device) as loader:
            for i in range(len(loader)):
                sample = loader.get()
                sample = {k: v.to(baseline.device) if isinstance(v, torch.Tensor) else v for k, v in sample.items()}
                image = sample["image"]

                torch.cuda.synchronize()
                with torch.inference_mode():
                    start = time.time()
                    pred = baseline.infer_for_evaluation(image, sample["intrinsics"]) if oracle_mode else baseline.infer_for_evaluation(image)
                    torch.cuda.synchronize()
                    elapsed = time.time() - start

                metrics, misc = compute_metrics(pred, sample, vis=dump_pred or dump_gt)
                metrics["inference_time"] = elapsed
                metrics_list.append(metrics)

                dump_path = Path(output_path.replace(".json", "_dump"), f"{benchmark_name}", sample["filename"].replace(".zip", ""))
                if dump_pred:
                    _dump_pred(dump_path / "pred", image, metrics, misc, pred)
                if dump_gt:
                    _dump_gt(dump_path / "gt", image, sample)

                if i % 100 == 0 or i == len(loader) - 1:
                    Path(output_path).write_text(json.dumps({**all_metrics, benchmark_name: key_average(metrics_list)}, indent=4))

        all_metrics[benchmark_name] = key_average(metrics_list)

    all_metrics["mean"] = key_average(list(all_metrics.values()))
    Path(output_path).write_text(json.dumps(all_metrics, indent=4))


def _rgb_u8(image):
    import numpy as np
    return (image.cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)


def _fov_json(path, intrinsics, key_name):
    import numpy as np
    from moge_amd.metrics import intrinsics_to_fov
    fov_x, fov_y = intrinsics_to_fov(intrinsics)
    with open(path / key_name, "w") as f:
        json.dump({"fov_x": np.rad2deg(fov_x.item()), "fov_y": np.rad2deg(fov_y.item()), "intrinsics": intrinsics.cpu().numpy().tolist()}, f)


def _dump_pred(path: Path, image, metrics, misc, pred):
    import numpy as np
    from PIL import Image
    from moge_amd.io import colorize_depth, colorize_normal, save_exr
    path.mkdir(parents=True, exist_ok=True)
    Image.fromarray(_rgb_u8(image)).save(path / "image.jpg", quality=95)
    with (path / "metrics.json").open("w") as f:
        json.dump(metrics, f, indent=4)
    if "pred_points" in misc:
        save_exr(path / "points.exr", misc["pred_points"].cpu().numpy().astype(np.float32))
    if "pred_depth" in misc:
        depth = misc["pred_depth"].cpu().numpy()
        if "mask" in pred:
            depth = np.where(pred["mask"].cpu().numpy(), depth, np.inf)
        Image.fromarray(colorize_depth(depth)).save(path / "depth.png")
    if "mask" in pred:
        Image.fromarray((pred["mask"].cpu().numpy() * 255).astype(np.uint8)).save(path / "mask.png")
    if "normal" in pred:
        Image.fromarray(colorize_normal(pred["normal"].cpu().numpy())).save(path / "normal.png")
    if "intrinsics" in pred:
        _fov_json(path, pred["intrinsics"], "fov.json")


def _dump_gt(path: Path, image, sample):
    import numpy as np
    from PIL import Image
    from moge_amd.io import colorize_depth, colorize_normal, save_exr
    path.mkdir(parents=True, exist_ok=True)
    Image.fromarray(_rgb_u8(image)).save(path / "image.jpg", quality=95)
    if "points" in sample:
        save_exr(path / "points.exr", sample["points"].cpu().numpy().astype(np.float32))
    if "depth" in sample:
        Image.fromarray(colorize_depth(sample["depth"].cpu().numpy(), mask=sample["depth_mask"].cpu().numpy())).save(path / "depth.png")
    if "normal" in sample:
        Image.fromarray(colorize_normal(sample["normal"].cpu().numpy())).save(path / "normal.png")
    if "depth_mask" in sample:
        Image.fromarray((sample["depth_mask"].cpu().numpy() * 255).astype(np.uint8)).save(path / "mask.png")
    if "intrinsics" in sample:
        _fov_json(path, sample["intrinsics"], "info.json")


if __name__ == "__main__":
    main()
