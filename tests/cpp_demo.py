"""What the tests of the C++ drop-in library share: building libfeature_detector.so and the headless demos
of tests/cpp (feature_detector_amd/api/Makefile), running a demo and reading the JSON lines it prints."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feature_detector_amd", "lib")
# a child process with this environment sees no GPU
NO_GPU_ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])


def records(stdout):
    """The JSON lines of a demo's output, in order."""
    return [json.loads(line) for line in stdout.splitlines() if line.startswith("{")]


def run(prog, *args, env=None, timeout=300):
    """Runs demo `prog`, which must exit with 0: its records by their "test" field (a record without one by
    its position), and its stderr."""
    out = subprocess.run([os.path.join(LIB, prog), *map(str, args)], capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr
    return {r.get("test", i): r for i, r in enumerate(records(out.stdout))}, out.stderr


def exported(symbol):
    """Whether libfeature_detector.so exports a symbol whose demangled name contains `symbol`."""
    nm = subprocess.run(["nm", "-DC", os.path.join(LIB, "libfeature_detector.so")], capture_output=True, text=True).stdout
    return symbol in nm
