# builds tools/probes/bin/libclover_<name>.so with ONE source of clover_amd/csrc compiled under the given -D sets (the other
# objects come from the regular bf16 build): build_wg_variants.sh [source] name1 "-DX" name2 "-DY -DZ" ...
#   source: a file name without .hip (default gemm_wgrad), e.g.   build_wg_variants.sh gemm_nt lab "-DGN_LAB"
# gives tools/probes/bin/libclover_lab.so, the library with the forced GEMM tile classes (CLV_GEMM_TILE) that
# gemm_tiles.py / gemm_sweep.py load through CLOVER_HALF=bf16 CLOVER_LIB_PATH=tools/probes/bin/libclover_lab.so
set -e
src=gemm_wgrad
if [ $(( $# % 2 )) -eq 1 ]; then src=$1; shift; fi
mkdir -p tools/probes/bin
make -C clover_amd/csrc -j8 > /dev/null
while [ $# -ge 2 ]; do
  n=$1; d=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics $d -c clover_amd/csrc/$src.hip -o tools/probes/bin/${src}_$n.o
  objs=$(ls clover_amd/csrc/build/*.o | grep -v /$src.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs tools/probes/bin/${src}_$n.o -o tools/probes/bin/libclover_$n.so
  echo built $n
done
