"""CPU. The PCG jump-ahead of the ray-major ambient-occlusion layout (rt_device.h pcg_jump / pcg_jump_of / PcgJumpTable,
frame_kernels.h k_ao<1>): lane i starts at draw 3i of its pixel's sequence, so for every i < 64 the jump must land exactly
where 3i sequential uniform() steps land (common/rng.hpp:8-58), from any (state, inc)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "rt_device.h"
using namespace rt;
static constexpr PcgJumpTable<64, 3> kTable{};
int main(int argc, char** argv)
{
    int bad = 0, checked = 0;
    for (int a = 1; a + 1 < argc; a += 2)
    {
        PCG r0;
        r0.state = strtoull(argv[a], nullptr, 10);
        r0.inc = strtoull(argv[a + 1], nullptr, 10) | 1ull;
        PCG seq = r0;
        for (int i = 0; i < 64; ++i)
        {
            const PCG j = pcg_jump(r0, kTable.e[i]);
            const PCG k = pcg_jump(r0, pcg_jump_of(3 * i));
            PCG jj = j, ss = seq;
            for (int d = 0; d < 3; ++d) bad += jj.uniform() != ss.uniform(); /* the three draws of ray i */
            bad += j.state != seq.state || j.inc != seq.inc || k.state != seq.state;
            ++checked;
            seq.uniform(); seq.uniform(); seq.uniform();
        }
    }
    printf("checked %d bad %d\n", checked, bad);
    return bad != 0;
}
"""


def test_pcg_jump_ahead_equals_sequential_draws(tmp_path):
    src = tmp_path / "jump.cpp"
    exe = tmp_path / "jump"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src)], check=True,
                   capture_output=True, timeout=300)
    rng = np.random.default_rng(2024)
    words = rng.integers(0, 2**64, size=(16, 2), dtype=np.uint64)
    args = [str(int(w)) for pair in words for w in pair]
    args += ["0", "1", str(2**64 - 1), str(2**64 - 1)]  # the zero state and the all-ones corner
    p = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "checked 1152 bad 0" in p.stdout, p.stdout + p.stderr


def test_pcg_init_of_the_ao_pixels_is_what_the_jump_starts_from(tmp_path):
    """pcg_init(0, hashPCG3(x, y, 42)) (04_ao.cu:42) followed by 3i draws == the jump from the initialised generator."""
    src = tmp_path / "init.cpp"
    exe = tmp_path / "init"
    src.write_text(r"""
#include <cstdio>
#include "rt_device.h"
using namespace rt;
int main()
{
    int bad = 0;
    for (uint32_t y = 0; y < 40; y += 7)
        for (uint32_t x = 0; x < 40; x += 3)
        {
            const PCG r0 = pcg_init(0u, hashPCG3(x, y, 42u));
            PCG seq = r0;
            for (int i = 0; i < 64; ++i)
            {
                PCG j = pcg_jump(r0, pcg_jump_of(3 * i));
                for (int d = 0; d < 3; ++d) bad += j.uniformf() != seq.uniformf();
            }
        }
    printf("bad %d\n", bad);
    return bad != 0;
}
""")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src)], check=True,
                   capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "bad 0" in p.stdout, p.stdout + p.stderr
