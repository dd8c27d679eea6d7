#!/bin/bash
# The --batch measurement: wall time of one process per family in a plain shell loop against `--batch --batch_cells 1`
# (one process, nothing shared) and the default `--batch`, for the default flow and for `--fasta -t`.
# NFAM=n: fewer families (a trial run).
# Usage: measure_batch.sh PGMSA SOLO_PGMSA WORKDIR OUT [RUNS=3] [SOLO_RUNS=1]   (SOLO_PGMSA: the driver the loop runs, e.g. a build of the parent commit)
set -o pipefail
PGMSA=$1; SOLO=$2; W=$3; OUT=$4; RUNS=${5:-3}; SOLO_RUNS=${6:-1}
HERE=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$W" "$OUT"
python "$HERE/make_batch_set.py" "$W" "${NFAM:-512}" 16 300 4242 || exit 1
now() { date +%s.%N; }
since() { awk -v a="$1" -v b="$(now)" 'BEGIN { printf "%.3f", b - a }'; }
# guide trees for the -t flow: one batch run (not timed), then a list with the tree column
awk -F'\t' '{print $1 "\t" $1 ".nwk"}' "$W/families.list" > "$W/trees.list"
timeout -k 10 300 "$PGMSA" --batch "$W/trees.list" -T -i 0 || exit $?
awk -F'\t' '{print $1 "\t" $2 "\t" $1 ".nwk"}' "$W/families.list" > "$W/families_t.list"
for flow in default t; do
    list="$W/families.list"; [ $flow = t ] && list="$W/families_t.list"
    for r in $(seq 1 "$SOLO_RUNS"); do
        t0=$(now)
        while read -r fa; do
            if [ $flow = t ]; then timeout -k 10 60 "$SOLO" --fasta -t "$fa.nwk" "$fa" > "$W/out/solo.out" || exit $?
            else timeout -k 10 60 "$SOLO" --fasta "$fa" > "$W/out/solo.out" || exit $?; fi
        done < "$W/families.txt"
        echo "$flow loop run $r: $(since "$t0") s" | tee -a "$OUT/batch_walls.txt"
    done
    for mode in own shared; do
        extra=""; [ $mode = own ] && extra="--batch_cells 1"
        for r in $(seq 1 "$RUNS"); do
            t0=$(now)
            timeout -k 10 300 "$PGMSA" --batch "$list" --fasta --stats $extra 2>> "$OUT/batch_${flow}_${mode}_stats.jsonl" || exit $?
            echo "$flow batch $mode run $r: $(since "$t0") s" | tee -a "$OUT/batch_walls.txt"
        done
    done
done
