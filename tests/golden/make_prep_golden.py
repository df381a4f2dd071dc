"""Golden vectors of the reference's portfolio preparation: `abs_port_norm`
(madigan/modelling/algorithm/utils.py:31-41) driven on the CPU exactly as the
agents' prep_state_tensors drives it (dqn.py:188-195, sac.py:237-244):

    port = torch.as_tensor(state.portfolio[:, -1], dtype=torch.float32)
    port = abs_port_norm(port)

    python tests/golden/make_prep_golden.py

The reference checkout is found as make_golden.py finds it ($MADIGAN_REFERENCE);
utils.py is imported by path (it needs only numpy and torch).  Per asset count
A in {1, 8, 64}: `port_A<A>` (R, W, A+1) float64 portfolio windows -- cash
first, as ledgerNormedFull -- and `out_A<A>` (R, A+1) float32, the reference's
result for the windows' last rows.  The rows: long-only weights, shorts,
leveraged rows with entries > 1, all cash, a zero row, random rows of mixed
magnitudes.  Inputs and outputs only go to tests/golden/prep_state_vectors.npz.
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MADIGAN_REFERENCE", "/root/reference")
ASSETS = (1, 8, 64)
W = 3


def reference_utils():
    path = os.path.join(REF, "madigan", "modelling", "algorithm", "utils.py")
    spec = importlib.util.spec_from_file_location("madigan_algorithm_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rows_for(A, rng):
    P = A + 1
    rows = []
    for _ in range(6):  # long only: weights sum to 1
        w = rng.random(P)
        rows.append(w / w.sum())
    for _ in range(6):  # shorts: negative asset weights, cash above 1
        a = -rng.random(A) * rng.choice([0.05, 0.5, 2.0])
        rows.append(np.concatenate([[1.0 - a.sum()], a]))
    for _ in range(6):  # leveraged: asset entries > 1, cash negative
        a = 1.0 + 4.0 * rng.random(A)
        rows.append(np.concatenate([[1.0 - a.sum()], a]))
    for _ in range(4):  # long and short together, leveraged
        a = rng.standard_normal(A) * 3.0
        rows.append(np.concatenate([[1.0 - a.sum()], a]))
    for _ in range(4):  # mixed magnitudes
        rows.append(rng.standard_normal(P) * 10.0 ** rng.integers(-12, 6, P))
    cash = np.zeros(P)
    cash[0] = 1.0
    rows.append(cash)       # all cash
    rows.append(np.zeros(P))  # a zero row (the padding of a window that is not full)
    one = np.zeros(P)
    one[-1] = -2.5
    rows.append(one)        # a single short entry
    return np.stack(rows)


def main():
    utils = reference_utils()
    rng = np.random.default_rng(0x70726570)
    data = {"assets": np.array(ASSETS, dtype=np.int64)}
    for A in ASSETS:
        last = rows_for(A, rng)
        port = rng.standard_normal((last.shape[0], W, A + 1))  # earlier rows: never read
        port[:, -1] = last
        ref = utils.abs_port_norm(torch.as_tensor(port[:, -1], dtype=torch.float32))
        assert ref.dtype == torch.float32 and ref.device.type == "cpu"
        data[f"port_A{A}"] = port
        data[f"out_A{A}"] = ref.numpy()
    path = os.path.join(HERE, "prep_state_vectors.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
