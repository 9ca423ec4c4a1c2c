"""Digest of the device code of every object of libpromonet_hip.so.

For each object of `make objs`: dump the .hip_fatbin section, unbundle the
gfx950 code object and print the sha256 of its .text and of its .rodata. Two
builds of the same kernels give the same lines, so a change that claims to
leave the kernels alone shows it by equal listings before and after. The whole
code object is no use for that: the name of its __hip_cuid_* symbol changes
with every build. Hashes only; runs on the CPU.

    make -j16 && python scripts/device_code_digest.py [objects...]
"""
import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path('/opt/rocm/lib/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def run(tool, *args):
    subprocess.run([str(LLVM / tool), *map(str, args)], check=True)


def section_digest(code_object, section, scratch):
    out = scratch / section.lstrip('.')
    out.write_bytes(b'')    # (a section that is absent dumps nothing)
    subprocess.run(
        [str(LLVM / 'llvm-objcopy'), f'--dump-section={section}={out}',
         str(code_object), str(scratch / 'discard')],
        check=False, capture_output=True)
    return hashlib.sha256(out.read_bytes()).hexdigest()


def digests(obj):
    with tempfile.TemporaryDirectory() as name:
        scratch = Path(name)
        fatbin, code_object = scratch / 'fatbin', scratch / 'gfx950.co'
        run('llvm-objcopy', f'--dump-section=.hip_fatbin={fatbin}', obj,
            scratch / 'discard')
        run('clang-offload-bundler', '--type=o', '--unbundle',
            f'--targets={TARGET}', f'--input={fatbin}',
            f'--output={code_object}')
        return [section_digest(code_object, section, scratch)
                for section in ('.text', '.rodata')]


def main():
    objects = sys.argv[1:] or subprocess.run(
        ['make', '-s', 'objs'], cwd=ROOT, check=True, capture_output=True,
        text=True).stdout.split()
    for obj in objects:
        text, rodata = digests(ROOT / obj)
        print(f'{Path(obj).name:24} .text {text}  .rodata {rodata}')


if __name__ == '__main__':
    main()
