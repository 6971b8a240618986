"""bench.py with the fused linear-layer update picked by I2V_TUNE_FC_UPDATE (not an environment knob): the A/B of round 7.

    python tools/bench_ab.py --fc-update {0,1} [bench.py arguments]

Sets the key in this process, then runs bench.py's own main() unchanged (same process, same arguments)."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    args = sys.argv[1:]
    if len(args) < 2 or args[0] != "--fc-update":
        sys.exit("usage: tools/bench_ab.py --fc-update {0,1} [bench.py arguments]")
    mode = int(args[1])
    from i2vsgg_amd._lib import TUNE, lib
    if lib.i2v_set_tuning(TUNE["I2V_FC_UPDATE"], mode) != 0:
        sys.exit("I2V_FC_UPDATE=%d refused: %s" % (mode, lib.i2v_last_error().decode()))
    sys.argv = [os.path.join(ROOT, "bench.py")] + args[2:]
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
