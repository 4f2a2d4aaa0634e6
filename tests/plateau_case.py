"""Crafted loss sequences for the ReduceLROnPlateau rule of the decoder pre-fit (``sings_amd.avatar_init.PlateauRule`` on the host,
``DevicePlateau`` on the GPU), and torch's own scheduler run over them."""
import numpy as np
import torch

REFERENCE_LRS = (0.00016 * 2.0, 1e-3, 1e-3, 1e-3)       # cfg.human.lr: position_init * smpl_spatial, vembed, geometry, appearance


def sequences(patience):
    """-> [(name, base rates of the four groups, fp32 losses)].  Every value is an fp32 number: the device reads the loss from an fp32
    scalar, the host rule and torch get the same number as a double."""
    P = int(patience)
    cases = []
    # a plateau longer than the patience, long enough for two reductions in a row
    cases.append(("plateau", REFERENCE_LRS, [1.0] * (2 * (P + 1) + 3)))
    # an improvement by less than the relative threshold (1e-4): not an improvement; three such steps together are one
    cases.append(("below_threshold", REFERENCE_LRS, [0.7 * (1.0 - 5e-5) ** i for i in range(3 * (P + 1) + 2)]))
    cases.append(("never_enough", REFERENCE_LRS, [0.7] + [0.7 * (1.0 - 0.9e-4)] * (P + 4)))
    # an improvement exactly at step patience + 1 after the best: the count reaches the patience and is reset, no reduction; then a
    # plateau of patience + 1 steps reduces exactly at its last one
    cases.append(("just_in_time", REFERENCE_LRS, [1.0] + [1.0] * P + [0.5] + [0.5] * (P + 1) + [0.5, 0.25]))
    # two reductions in a row with an improvement between runs, then NaN (never better)
    cases.append(("two_in_a_row", REFERENCE_LRS, [2.0, 1.0] + [1.5] * (2 * (P + 1)) + [0.9] + [float("nan")] * (P + 2)))
    # a group whose rate is so small that `old - new > eps` (1e-8) stops its reduction: 3e-8 -> 1.5e-8 -> stays
    cases.append(("eps_stops", (3e-8, 1e-3, 1e-3, 1e-3), [1.0] * (3 * (P + 1) + 2)))
    return [(n, tuple(lrs), np.asarray(v, np.float32)) for n, lrs, v in cases]


def torch_rates(base_lrs, losses, patience, factor=0.5):
    """The rates of every group after each ``scheduler.step(loss)`` of torch's ReduceLROnPlateau on a dummy optimiser."""
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in base_lrs]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, base_lrs)])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=patience, factor=factor)
    rows = []
    for x in losses:
        sch.step(float(x))
        rows.append([float(g["lr"]) for g in opt.param_groups])
    return rows
