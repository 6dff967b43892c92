cd "$(dirname "$0")/.." || exit 2
R=$PWD; O=$(realpath -m "${OMG_OUT:-measurements}"); mkdir -p "$O"; export TMPDIR=/tmp
for i in 1 2; do
  OMG_NO_RHS_SHIFT=1 timeout -k 10 120 python bench.py --full --no-cpu-baseline --steps 20 > "$O/ab_off_$i.log" 2>&1 || exit $?
  timeout -k 10 120 python bench.py --full --no-cpu-baseline --steps 20 > "$O/ab_on_$i.log" 2>&1 || exit $?
done
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace -d "$O/prof_on" -o run --output-format csv -- python3 "$R/bench.py" --steps 3 --warmup 1 --full --no-cpu-baseline --no-profile-pass) > "$O/prof_on.log" 2>&1
