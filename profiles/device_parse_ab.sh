#!/bin/bash
# `taxor search --device-parse` A/B on the RefSeq-class synthetic index (docs/EXPERIMENTS.md, "Record scanning on the device"):
# plain four-line FASTQ and plain FASTA of 10-kb reads; this build without and with the switch (twice each) and another build's
# CLI without it as the baseline.  Every leg has its own time limit and a failure ends the run.  Raw outputs: profiles/device_parse/.
# usage: profiles/device_parse_ab.sh <baseline taxor binary> [reads=1048576] [output directory=profiles/device_parse]
set -o pipefail
cd "$(dirname "$0")/.."
BASE=${1:?baseline taxor binary}
N=${2:-1048576}
OUT=${3:-profiles/device_parse}
mkdir -p "$OUT"
for fmt in fastq fasta; do
  log=$OUT/measure_${fmt}_setup.txt
  TAXOR_E2E_KEEP=1 TAXOR_E2E_RUNS=16 TAXOR_E2E_FORMAT=$fmt timeout -k 10 500 python profiles/cli_e2e_class.py refseq "$N" > "$log" 2>&1
  rc=$?; tail -4 "$log"; [ $rc -ne 0 ] && exit $rc
  dir=$(grep '^kept: ' "$log" | sed 's/^kept: //')
  [ -d "$dir" ] || exit 9
  for leg in host device parent host2 device2; do
    case $leg in
      host|host2) bin=taxor_amd/taxor; sw="";;
      device|device2) bin=taxor_amd/taxor; sw="--device-parse";;
      parent) bin=$BASE; sw="";;
    esac
    out=$OUT/measure_${fmt}_${leg}.txt
    TAXOR_TUNING=1 TAXOR_CLI_TRACE=1 TAXOR_FASTX_TRACE=1 timeout -k 10 150 "$bin" search --index-file "$dir/refseq.hixf" --query-file "$dir/reads.fastq" \
        --output-file "$dir/out_$leg.tsv" --threads 16 $sw > "$out" 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then tail -5 "$out"; rm -rf "$dir"; exit $rc; fi
    cmp "$dir/out_$leg.tsv" "$dir/out.tsv" >> "$out" 2>&1 && echo "TSV identical to the reference run" >> "$out"
    grep -E "search phase|device-parse|fastx_scan|TSV identical" "$out" | cut -c1-260
    rm -f "$dir/out_$leg.tsv"
  done
  rm -rf "$dir"
done
