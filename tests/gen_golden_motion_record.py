"""TEST INFRASTRUCTURE -- golden for the state dump of phc_amd/motion_record.py: `body_quat` from the reference's OWN code.

Run where the reference checkout is (oracle/ref_shim.py finds it):  python tests/gen_golden_motion_record.py   -> tests/golden/motion_record.npz

`_write_states_to_file` (phc/env/tasks/humanoid_im.py:450) forms `body_quat = cat([root_states[:, None, 3:7], torch_utils.exp_map_to_quat(dof_pos.reshape(B, -1, 3))])`;
the statement is run here with the reference's `torch_utils.exp_map_to_quat` on 64 frames of an SMPL-sized DoF state (23 joints): exp maps of angles over
[0, 2 pi), the zero map, maps below and above the function's 1e-5 mask, and one of angle pi - 0.05.  The file holds arrays only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()

OUT = os.path.join(ROOT, "tests", "golden", "motion_record.npz")
F = np.float32
B, J = 64, 23


def main():
    torch_utils = ref_shim.ref_module("phc.utils.torch_utils")
    rng = np.random.default_rng(411)
    axis = rng.standard_normal((B, J, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    angle = rng.uniform(0.0, 2 * np.pi, (B, J))
    angle[np.abs(angle - np.pi) < 1e-2] = np.pi + 0.5      # (normalize_angle returns +pi or -pi at pi)
    angle[0, :5] = [0.0, 2e-6, 6e-5, np.pi - 0.05, 1e-3]
    dof_pos = (axis * angle[..., None]).astype(F).reshape(B, J * 3)
    q = rng.standard_normal((B, 4))
    root_quat = (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F)
    root_states = np.concatenate([rng.standard_normal((B, 3)).astype(F), root_quat, rng.standard_normal((B, 6)).astype(F)], axis=1)
    root_states_seg, dof_pos_seg = torch.from_numpy(root_states), torch.from_numpy(dof_pos)
    body_quat = torch.cat([root_states_seg[:, None, 3:7], torch_utils.exp_map_to_quat(dof_pos_seg.reshape(B, -1, 3))], dim=1)
    np.savez_compressed(OUT, dof_pos=dof_pos, root_quat=root_quat, body_quat=body_quat.numpy().astype(F))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
