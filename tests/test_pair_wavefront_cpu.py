"""Where the pair-HMM wavefront stands, on the CPU -- no GPU.

tools/pair_wavefront_host_check.cpp runs the kernels' own text (csrc/pair_geom.h: PaGeom and PaStripe, from which paWalkForward
and pcBackwardPair take every stripe, step and lane) under ASan and UBSan: over the aligner's shapes, eight bands and three
numbers of duplication lengths the enumeration must stand on every cell of dnas::PairBand exactly once and on nothing else, file
it where PaGeom::wordAt finds it, meet every neighbour a cell reads at the step and lane the walks take it from, and meet the same
cell at the same place going back.  The test builds and runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# how the program's one summary line begins when every check held (the sizes of its run follow)
HOST_CHECK_LINE = b"pair wavefront host check: ok (240 cases, "


def test_wavefront_geometry_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pair_wavefront_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "pair_wavefront_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and HOST_CHECK_LINE in r.stdout, (r.stdout.decode(), r.stderr.decode()[-4000:])
