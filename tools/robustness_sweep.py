#!/usr/bin/env python3
"""Sweep a trained MSACL controller over sensor / actuator noise levels in closed loop
(trainer/robustness_auditor.py): load an apprfunc_*.pkl, follow the loop from the same drawn
initial states under every level (the Cartesian product of --obs-sigma x --act-sigma x --act-bias),
print one JSON line per level, optionally save the per-env arrays.

Usage: python tools/robustness_sweep.py RUN/apprfunc/apprfunc_N.pkl [--config RUN/config.json]
           [--obs-sigma 0 0.01 0.05] [--act-sigma 0 0.1] [--act-bias 0 0.2]
           [--trajectories 4096] [--horizon 1000] [--tail-window 100] [--settle-frac 0.01]
           [--ball-factor 1.0] [--independent-noise] [--device cpu] [--out sweep.npz]
obs_sigma is in observation units; act_sigma and act_bias are fractions of the action box's
half-width. The config defaults to config.json of the run the checkpoint belongs to."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("apprfunc")
    ap.add_argument("--config")
    ap.add_argument("--obs-sigma", type=float, nargs="+", default=[0.0])
    ap.add_argument("--act-sigma", type=float, nargs="+", default=[0.0])
    ap.add_argument("--act-bias", type=float, nargs="+", default=[0.0])
    ap.add_argument("--trajectories", type=int, default=1024)
    ap.add_argument("--horizon", type=int)
    ap.add_argument("--tail-window", type=int, default=100)
    ap.add_argument("--settle-frac", type=float, default=0.01)
    ap.add_argument("--ball-factor", type=float, default=1.0)
    ap.add_argument("--independent-noise", action="store_true",
                    help="every env its own noise realisation (default: levels share them)")
    ap.add_argument("--device")
    ap.add_argument("--out")
    a = ap.parse_args()

    import numpy as np
    import torch
    import msacl_amd  # noqa: F401
    from msacl_amd.create_pkg.create_auditor import create_auditor

    cfg_path = a.config or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(a.apprfunc))), "config.json")
    with open(cfg_path, encoding="utf-8") as f:
        args = json.load(f)
    for k in ("action_high_limit", "action_low_limit"):
        args[k] = np.asarray(args[k], np.float32)
    if a.device is not None:
        args["device"] = a.device
    args.pop("auditor_name", None)
    auditor = create_auditor("robustness_auditor", **args)
    auditor.load_state_dict(torch.load(a.apprfunc, weights_only=True))
    auditor.networks.to(auditor.device).eval()
    levels = [dict(obs_sigma=so, act_sigma=sa, act_bias=b)
              for so, sa, b in itertools.product(a.obs_sigma, a.act_sigma, a.act_bias)]
    res = auditor.sweep(levels, trajectories=a.trajectories, horizon=a.horizon, tail_window=a.tail_window,
                        settle_frac=a.settle_frac, ball_factor=a.ball_factor, common_noise=not a.independent_noise)
    auditor.close()
    for lv in res["levels"]:
        print(json.dumps(dict(env=args["env_name"], **lv)))
    if a.out:
        arrays = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items() if k != "levels"}
        arrays["levels_json"] = np.array(json.dumps(res["levels"]))
        np.savez(a.out, **arrays)


if __name__ == "__main__":
    main()
