import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "event-retrival-in-video-learning-transferable-visual-model-from-supervised-natural-language_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

# the parity tests run on deterministic random-init weights of the real
# architectures (no checkpoints offline); the product refuses them unless asked
os.environ.setdefault("MICLIP_SYNTHETIC_WEIGHTS", "1")

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through the HIP C-ABI)")
    config.addinivalue_line("markers", "slow: full-size model cases")


@functools.lru_cache(maxsize=4)
def state_dict(name):
    from miclip import config, weights
    return weights.make_state_dict(config.get_config(name))


@pytest.fixture(scope="session")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def golden(name):
    """A fixture under tests/golden; a .npz whose largest array was stored beside it as
    <stem>.part2.npz (make_golden.py save_split: no file above 1 MiB) is read as one mapping."""
    d = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    part2 = os.path.join(GOLDEN, name[:-4] + ".part2.npz")
    if name.endswith(".npz") and os.path.exists(part2):
        d = {**{k: d[k] for k in d.files}, **np.load(part2, allow_pickle=False)}
    return d
