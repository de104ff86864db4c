#!/bin/bash
# builds build_abl/lib_<name>.so: cnf_step3.hip (build_abl/src/cnf_step3_<name>.hip instead, where there is one) compiled with
# $EXTRA, e.g. EXTRA=-DS3_STAMPS, + the current objects of the other sources (run make first).  Use: CNFHIP_LIB=build_abl/lib_<name>.so
set -e
cd "$(dirname "$0")/../continuousnf.jl_amd/csrc"
mkdir -p ../../build_abl
for v in "$@"; do
  src=cnf_step3.hip
  if [ -f ../../build_abl/src/cnf_step3_$v.hip ]; then src=../../build_abl/src/cnf_step3_$v.hip; fi   # (the .inc files it includes are found through -I.)
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result -ffp-contract=fast -I. ${EXTRA:-} -c $src -o ../../build_abl/cnf_step3_$v.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build_abl/lib_$v.so ../../build_abl/cnf_step3_$v.o $(ls *.o | grep -v '^cnf_step3\.o$') -ldl
  echo "built lib_$v.so"
done
