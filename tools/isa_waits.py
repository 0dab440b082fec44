"""Loads, vmcnt waits and branches per kernel from the device assembly of every csrc/*.hip (esr_nerf_amd/build.py:
device_asm): a kernel whose wait count approaches its load count issues its loads one round trip at a time (DESIGN.md
section 4, "conditional loads serialise").
   python tools/isa_waits.py"""
import re,subprocess,sys,os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esr_nerf_amd.build import device_asm, sources      # noqa: E402
for f in sources():
    name=None; stats={}
    for line in open(device_asm(f)):
        m=re.match(r'^(_Z\w+):',line)
        if m: name=m.group(1); stats[name]=dict(ld=0,w0=0,w=0,br=0,v=0); continue
        if line.startswith('.Lfunc_end'): name=None
        if not name: continue
        st=stats[name]
        if 'global_load' in line or 'buffer_load' in line or 'flat_load' in line: st['ld']+=1
        if 's_waitcnt' in line and 'vmcnt(0)' in line: st['w0']+=1
        if 's_waitcnt' in line and 'vmcnt' in line: st['w']+=1
        if 's_cbranch' in line: st['br']+=1
        if re.match(r'\s+v_',line): st['v']+=1
    for n,st in stats.items():
        if st['ld']>=8:
            d=subprocess.run(['c++filt',n],capture_output=True,text=True).stdout.strip()[:100]
            print(f"{f:16s} ld {st['ld']:4d} vmcnt0 {st['w0']:4d} vmcnt {st['w']:4d} br {st['br']:4d} valu {st['v']:5d}  {d}")
