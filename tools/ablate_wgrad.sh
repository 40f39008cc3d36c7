# wgrad ablation builds (numerically wrong by construction; timing only): libmzba_abl1.so = no next-stage global
# loads, libmzba_abl3.so = no per-tap B fragment reloads; per-launch timings beside the product build. The ablation
# switch is no longer in the sources (csrc/wgrad.hip): build the two libraries from a copy of the tree with
# profiles/r06/wgrad_abl/wgrad_ablate_retired.patch put back (patch -R -p1), -DMZBA_WGRAD_ABLATE=1 and =3
set -e
D=gpurun_out/wgrad_abl; mkdir -p $D
for L in libmzba.so libmzba_abl1.so libmzba_abl3.so libmzba.so; do
  MZBA_LIB=muzero-breakout_amd/mzba/$L timeout -k 10 200 python tools/bench_wgrad_segs.py | sed "s/^{/{\"lib\": \"$L\", /" >> $D/segs.jsonl
done
