"""The launch stream of one EMRT eval forward and one train step, as comparable text (developer tool, CPU, no library needed).

usage: PYTHONPATH=<checkout under test> python tools/launch_log.py --backbone resnet18 --out /tmp/a    # -> /tmp/a.eval.txt, /tmp/a.train.txt

The model of the checkout that PYTHONPATH names (this one without it) runs on the recording stand-in for the C-ABI (tests/fake_abi.py of THAT checkout);
the canonical text is made by this tree's tests/fake_abi.canonical_log, so checkouts older than it can be compared too.  A refactor of the host code
leaves both files byte-identical.
"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)            # (behind PYTHONPATH: the checkout under test wins)
import torch                     # noqa: E402

from tests import fake_abi       # noqa: E402
from tests.test_host_logic_cpu import _place      # noqa: E402


def _own(*path):
    """a module of THIS tree, whatever PYTHONPATH says"""
    spec = importlib.util.spec_from_file_location("launch_log_" + path[-1][:-3], os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


canonical_log, binding = _own("tests", "fake_abi.py").canonical_log, _own("emrt_amd", "_lib.py")

ap = argparse.ArgumentParser()
ap.add_argument("--backbone", choices=["resnet18", "resnet50"], default="resnet18")
ap.add_argument("--out", default="launch_log", help="prefix of the two files written")
args = ap.parse_args()

from emrt_amd.src.models.emrt import EMRT                               # noqa: E402
from emrt_amd.src.models.losses import MixSoftmaxCrossEntropyLoss       # noqa: E402
from emrt_amd.src.models.solver import Momentum, PolynomialDecay        # noqa: E402

fake = fake_abi.install()
torch.manual_seed(0)
m = _place(EMRT(num_classes=6, backbone=args.backbone))
x, lab = torch.randn(2, 3, 64, 64), torch.randint(0, 6, (2, 64, 64))
m.eval()
m(x)
logs = {"eval": canonical_log(fake.calls, binding)}
fake.calls.clear()
m.train()
opt = Momentum(m, PolynomialDecay(0.01, 100), 0.9, 1e-4, 1.0)
m.clear_gradients()
MixSoftmaxCrossEntropyLoss()(m(x), lab).backward()
opt.step()
logs["train"] = canonical_log(fake.calls, binding)
for phase, text in logs.items():
    with open("%s.%s.txt" % (args.out, phase), "w") as f:
        f.write(text)
    print("%s.%s.txt: %d launches" % (args.out, phase, text.count("\n")))
