cd "$(dirname "$0")/.." || exit 2
R=$PWD; O=$(realpath -m "${OMG_OUT:-measurements}"); mkdir -p "$O"; export TMPDIR=/tmp
for i in 1 2 3; do
  OMG_NO_FUSE_DOWN=1 timeout -k 10 120 python bench.py --full --no-cpu-baseline --steps 20 > "$O/ab_off_$i.log" 2>&1 || exit $?
  timeout -k 10 120 python bench.py --full --no-cpu-baseline --steps 20 > "$O/ab_on_$i.log" 2>&1 || exit $?
done
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/prof_on" -o run --output-format csv -- python3 "$R/bench.py" --steps 5 --warmup 1 --full --no-cpu-baseline) > "$O/prof_on.log" 2>&1
