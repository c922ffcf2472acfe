"""
The gfx950 assembly that the build keeps beside the objects (csrc/Makefile, ASM_SRCS: -save-temps, the text the shipped object
was assembled from), for the host tests that check it: kernel names and private-segment (scratch) sizes.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, 'bayeslim_amd', 'lib', 'obj')


def read(name):
    """(assembly text, kernel symbols, private segment sizes) of csrc/<name>.hip in this build; builds the library if the
    file is not there yet"""
    path = os.path.join(OBJ, name + '-hip-amdgcn-amd-amdhsa-gfx950.s')
    if not os.path.exists(path):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'bayeslim_amd', 'csrc')], check=True, capture_output=True)
    asm = open(path).read()
    kernels = re.findall(r'\.amdhsa_kernel (\S+)', asm)
    sizes = [int(x) for x in re.findall(r'\.amdhsa_private_segment_fixed_size (\d+)', asm)]
    return asm, kernels, sizes
