#!/usr/bin/env python3
"""Audit the Lyapunov certificate of a trained MSACL controller in closed loop
(trainer/certificate_auditor.py): load an apprfunc_*.pkl, follow the deterministic closed loop
from drawn (or phase-plane grid) initial states, print the summary, optionally save the per-env
arrays.

Usage: python tools/audit_certificate.py RUN/apprfunc/apprfunc_N.pkl [--config RUN/config.json]
           [--states 65536] [--horizon 1000] [--grid I J --points 65 [--span S]] [--device cpu]
           [--out audit.npz]
The config defaults to config.json of the run the checkpoint belongs to (its networks' sizes, the
env, n_step, lya_eta, alpha1 / alpha2 and the reward / cost scales)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("apprfunc")
    ap.add_argument("--config")
    ap.add_argument("--states", type=int)
    ap.add_argument("--horizon", type=int)
    ap.add_argument("--grid", type=int, nargs=2, metavar=("I", "J"))
    ap.add_argument("--points", type=int, default=65)
    ap.add_argument("--span", type=float)
    ap.add_argument("--device")
    ap.add_argument("--out")
    a = ap.parse_args()

    import numpy as np
    import torch
    import msacl_amd  # noqa: F401
    from msacl_amd.create_pkg.create_auditor import create_auditor
    from msacl_amd.trainer.certificate_auditor import state_grid

    cfg_path = a.config or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(a.apprfunc))), "config.json")
    with open(cfg_path, encoding="utf-8") as f:
        args = json.load(f)
    for k in ("action_high_limit", "action_low_limit"):
        args[k] = np.asarray(args[k], np.float32)
    if a.states is not None:
        args["num_audit_states"] = a.states
    if a.device is not None:
        args["device"] = a.device
    auditor = create_auditor(args.pop("auditor_name", "certificate_auditor"), **args)
    auditor.load_state_dict(torch.load(a.apprfunc, weights_only=True))
    auditor.networks.to(auditor.device).eval()
    init = state_grid(args["env_name"], a.grid, a.points, a.span) if a.grid else None
    res = auditor.audit(initial_states=init, horizon=a.horizon)
    auditor.close()
    print(json.dumps(dict(env=args["env_name"], states=int(res["len"].numel()), **res["summary"])))
    if a.out:
        arrays = {k: v.cpu().numpy() for k, v in res.items() if k != "summary"}
        if init is not None:
            arrays["initial_states"] = init
        np.savez(a.out, **arrays)


if __name__ == "__main__":
    main()
