"""Records tests/golden/ref_pin.npz and tests/golden/ref_epic.npz: the compiled reference's answers to every call the pinning tests
(tests/test_oracle_pin.py, tests/test_epic.py) make, keyed by a digest of the call's inputs (tests/ref_replay.py) -- the SHA-256 of each
output where the oracle's counterpart reproduces it (checked here), the outputs themselves elsewhere.

Run where oracle/Makefile could build oracle/_ref (the reference sources present):
    python tests/golden/make_golden_pin.py
The tests run once against the live library with SFA_REF_RECORD=1; only the resulting data is committed.  Without a GPU the GPU-marked
epic test fails after its reference calls were recorded (it takes them first); that failure is expected here.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    sys.path.insert(0, ROOT)
    import oracle as orc
    if not orc.ref_available():
        raise SystemExit("oracle/_ref/libslowflow_ref.so is not built: build() where the reference sources are present")
    env = dict(os.environ, SFA_REF_RECORD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "", "tests/test_oracle_pin.py", "tests/test_epic.py"],
                       cwd=ROOT, env=env)
    for name in ("ref_pin", "ref_epic"):
        path = os.path.join(HERE, name + ".npz")
        print("%s: %s (%d bytes)" % (name, "written" if os.path.exists(path) else "MISSING", os.path.getsize(path) if os.path.exists(path) else 0))
    return r.returncode


if __name__ == "__main__":
    main()
