"""The owners of device memory (csrc/device_buffer.hpp: DevBuf, DevPool, the growth rules) under AddressSanitizer + UBSan in a
program of its own (tools/device_buffer_host_check.cpp), over a malloc-backed policy that counts and can fail an allocation; and
the rule that no other file of csrc/ allocates or frees device memory itself."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnastore_amd", "csrc")


def test_owners_under_sanitizers(tmp_path):
    """The header compiles with plain g++ (no HIP headers); every growth rule equals its formula, 2^31 x 64 included; reserve,
    reserveKeep and assign keep their promises with and without a failed allocation; moves leave the source empty; frees equal
    allocations and nothing is freed twice.  All of it over the debug allocation mode's wrapper (GuardedMem) with DNAS_DEBUG_ALLOC
    unset, the policy's call counts those of the program before the wrapper existed; then the mode itself: every byte of a new
    block and its guard band filled, reserveKeep's prefix kept and the rest filled, no map entry after a failed allocation or
    fill, stores at p[bytes] and p[bytes + 255] reported at the free with their size and offset and one at p[bytes - 1] not, a
    block of the mode still checked when it is freed outside it, moves freeing once, the map empty at the end."""
    exe = str(tmp_path / "device_buffer_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "device_buffer_host_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"device buffer host check: ok" in r.stdout, r.stderr.decode()


def test_only_the_header_allocates():
    calls = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree)\(")
    found = []
    for folder, _, names in os.walk(CSRC):
        for name in names:
            if name.endswith((".hip", ".h", ".hpp", ".cpp")) and name != "device_buffer.hpp":
                with open(os.path.join(folder, name), errors="replace") as f:
                    found += ["%s:%d" % (name, n) for n, line in enumerate(f, 1) if calls.search(line)]
    assert not found, found
