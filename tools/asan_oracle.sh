#!/bin/bash
# AddressSanitizer + UBSan run of the host scaffolding and the CPU oracle on golden fixtures (build container, CPU only:
# sanitizers are not available on the GPU pool).  Every output must match the committed fixture and the sanitizers must
# stay silent.
set -e
cd "$(dirname "$0")/.."
make -s -C oracle _build/pgmsa_oracle_asan
B=oracle/_build/pgmsa_oracle_asan G=tests/golden
chk() { local want=$1; shift; local got; got=$("$B" "$@" 2> oracle/_build/asan.err | md5sum | cut -d' ' -f1)
        [ "$got" = "$(md5sum < "$want" | cut -d' ' -f1)" ] && [ ! -s oracle/_build/asan.err ] && echo "ok   $*" || { echo "FAIL $*"; cat oracle/_build/asan.err; exit 1; }; }
chk $G/c1.nw_ml.tree -a -m -T -i 0 $G/c1.fa
chk $G/c1.out.fa --fasta --tree $G/c1.tree $G/c1.fa
chk $G/c1.cs.out.fa --fasta --tree $G/c1.tree --cs_profile $G/K50.lib $G/c1.fa
chk $G/cd1.out.fa --codon --fasta -t $G/cd1.tree $G/cd1.fa
chk $G/m1.out.fa --fasta --tree $G/m1.tree $G/m1.fa
chk $G/x1.out.fa --fasta --tree $G/x1.tree $G/x1.fa
rm -f oracle/_build/pgmsa_oracle_asan oracle/_build/pgm_oracle_asan.o oracle/_build/asan.err
echo "sanitizer run clean"
