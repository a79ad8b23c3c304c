"""The kernel handles compiled into librj.so, read from its ELF64 `.dynsym` (no external tools).

A `__global__` template instantiation leaves one host-side handle object per instantiation
(`STT_OBJECT`, e.g. `_ZN2rj6k_joinILi1ELi2ELi2ELi3ELi12ELi1EEEvNS_10JoinParamsE`); the
set of those named `rj::k_*` is what the kernel files (csrc/rj_*.hip) compiled.  The
ingest kernels live in anonymous namespaces and are not listed."""
import re
import shutil
import struct
import subprocess

SHT_DYNSYM = 11
STT_OBJECT = 1
KERNEL_RE = re.compile(r"^_ZN2rj\d+k_")


def dynsym_objects(path):
    """{name: st_value} of the defined STT_OBJECT symbols of an ELF64 little-endian file."""
    data = open(path, "rb").read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError(f"{path}: not a little-endian ELF64 file")
    e_shoff, = struct.unpack_from("<Q", data, 0x28)
    e_shentsize, e_shnum = struct.unpack_from("<HH", data, 0x3A)
    shdrs = []
    for i in range(e_shnum):
        # sh_name, sh_type, sh_flags, sh_addr, sh_offset, sh_size, sh_link, sh_info, sh_addralign, sh_entsize
        shdrs.append(struct.unpack_from("<IIQQQQIIQQ", data, e_shoff + i * e_shentsize))
    out = {}
    for sh in shdrs:
        if sh[1] != SHT_DYNSYM:
            continue
        off, size, link, entsize = sh[4], sh[5], sh[6], sh[9] or 24
        stroff = shdrs[link][4]
        for k in range(size // entsize):
            st_name, st_info, _other, st_shndx, st_value, _size = struct.unpack_from(
                "<IBBHQQ", data, off + k * entsize)
            if st_shndx == 0 or (st_info & 0xF) != STT_OBJECT:
                continue
            end = data.index(b"\0", stroff + st_name)
            out[data[stroff + st_name:end].decode()] = st_value
    return out


def kernel_handles(path):
    """Sorted mangled names of the `rj::k_*` kernel handles in the library."""
    return sorted(n for n in dynsym_objects(path) if KERNEL_RE.match(n))


def symbol_at(path, offset):
    """The kernel-handle name at `offset` from the library's base (the launch log's "+0x..." form)."""
    for name, value in dynsym_objects(path).items():
        if value == offset:
            return name
    return None


def family(mangled):
    """'k_join', 'k_pass_scatter', ... of a kernel handle's mangled name."""
    m = re.match(r"^_ZN2rj(\d+)", mangled)
    n = int(m.group(1))
    return mangled[m.end():m.end() + n]


def _targs(s, i):
    """Template arguments from s[i] (just past 'I') to the matching 'E' -> ([text], index past 'E')."""
    out = []
    while s[i] != "E":
        if s.startswith("Lb", i):  # bool literal
            out.append("true" if s[i + 2] == "1" else "false")
            i += 4
        elif s[i] == "L":  # Li<n>E, Li n<n>E (negative)
            m = re.match(r"L[a-z](n?)(\d+)E", s[i:])
            out.append(("-" if m.group(1) else "") + m.group(2))
            i += m.end()
        elif s.startswith("NS_", i):  # a class of namespace rj, maybe a template itself
            m = re.match(r"NS_(\d+)", s[i:])
            j = i + m.end()
            name = s[j:j + int(m.group(1))]
            j += int(m.group(1))
            if s[j] == "I":
                inner, j = _targs(s, j + 1)
                name += "<" + ",".join(inner) + ">"
            assert s[j] == "E", s
            out.append(name)
            i = j + 1
        else:
            raise ValueError(f"unexpected template argument at {s[i:]!r}")
    return out, i + 1


def short_name(mangled):
    """Compact readable name without a demangler: `k_join<1,2,2,3,12,1>`,
    `k_pass_scatter<3,SrcLoader<1,2,1>,1,true>` (template arguments as written in the source)."""
    m = re.match(r"^_ZN2rj(\d+)", mangled)
    n = int(m.group(1))
    i = m.end() + n
    name = mangled[m.end():i]
    if mangled[i] == "I":
        args, _ = _targs(mangled, i + 1)
        name += "<" + ",".join(args) + ">"
    return name


_DEMANGLED = {}


def readable(mangled):
    """`rj::k_join<1, 2, 2, 3, 12, 1>` through c++filt when it is on the PATH, else the mangled name."""
    if mangled in _DEMANGLED:
        return _DEMANGLED[mangled]
    text = mangled
    tool = shutil.which("c++filt")
    if tool:
        try:
            r = subprocess.run([tool, mangled], capture_output=True, text=True, timeout=10)
            if r.returncode == 0 and r.stdout.strip():
                text = r.stdout.strip()
                text = re.sub(r"^void ", "", text)
                text = re.sub(r"\(.*\)$", "", text)
        except (OSError, subprocess.SubprocessError):
            pass
    _DEMANGLED[mangled] = text
    return text
