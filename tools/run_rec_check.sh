# usage: bash tools/run_rec_check.sh OUT_DIR   (the recurrent-kernel tests, the cycle anatomy, one --full bench line)
O=${1:?usage: bash tools/run_rec_check.sh OUT_DIR}
timeout -k 10 300 python -m pytest tests -m gpu -x -q -k "recurrent or dyadic or golden or rnn or RNN or ann or bidirectional or long_seq" > $O/r2_t.log 2>&1; tail -3 $O/r2_t.log
SPARCH_HIP_LIB=sparch_amd/libsparch_hip_prof.so timeout -k 10 120 python tools/rec_prof.py > $O/r2_anat.txt 2>&1; tail -17 $O/r2_anat.txt
timeout -k 10 200 python bench.py --full --no-cpu-baseline > $O/r2_b.json 2> $O/r2_b.err; python -c "
import json
d=json.loads(open('$O/r2_b.json').read().strip().splitlines()[-1])
print(d['ms_per_step'], {k:v for k,v in d['kernels_ms_per_step'].items()})"
