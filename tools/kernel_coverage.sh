# usage (GPU box): bash tools/kernel_coverage.sh   -> gpurun_out/kernel_coverage.txt
# Which kernels of libicl_hip.so does the GPU suite + the three bench configurations launch?  (rocprofv3 kernel trace, names only)
# (volume_feed_kernel<1, false> and <4, false>, the AMOS data feed, are launched by tests/test_gpu_amos_feed.py: the (6, 6, 5) and (6, 6, 8) sweeps)
# (rank_count_kernel, rank_scan_kernel, rank_select_kernel of rankindex.h and volume_feed_kernel<1, true> and <4, true> of datafeed.h, the
#  pos/neg feed, are launched by tests/test_gpu_posneg_feed.py: the index and select tests, and the (6, 6, 5) and (6, 6, 8) batches)
# (volume_feed_affine_kernel<1, false>, <4, false>, <1, true> and <4, true> of datafeed.h, the affine stage of both feeds, are launched by
#  tests/test_gpu_affine_feed.py: the random-matrix cases on aligned and misaligned outputs, and the device-origin and non-finite tests at
#  (6, 6, 5), (6, 6, 8) and (8, 8, 8), the last with the affine path's 8 x 8 tiles)
# (intensity_noise_kernel<1> and <4>, intensity_blur_strided_kernel, intensity_blur_line_kernel<1> and <4>, intensity_stats_partial_kernel,
#  intensity_stats_finish_kernel, intensity_point_kernel<1> and <4> of intensity.h, the intensity stage of the 3-D feeds, are launched by
#  tests/test_gpu_intensity_feed.py: every check runs (7, 9, 10) for the one-voxel kernels and (8, 12, 16) for the quad kernels, and the
#  blur test repeats each shape on a batch that starts 4 bytes past a 16-byte boundary)
# (intensity_lowres_kernel<1> and <4>, intensity_lowres_copy_kernel<1> and <4> of intensity.h, the simulated low resolution of that stage,
#  are launched by tests/test_gpu_lowres_feed.py: (7, 9, 10), (9, 11, 13) and a misaligned (8, 12, 16) for the one-voxel kernels, (8, 12, 16)
#  and 96^3 for the quad kernels)
# (prefix_box_partial_kernel, prefix_box_finish_kernel, prefix_resample_kernel<1> and <4>, prefix_restore_kernel<uint8_t> and <long long> of
#  prefix.h, the AMOS cached prefix, are launched by tests/test_gpu_amos_prefix.py: the case list, the quad cases and the restore tests)
# (the surface-metric kernels of metrics_surface.h — surf_edt_axis2/1/0, surf_reduce, surf_radix<0..5>, surf_finish — are launched by
#  tests/test_gpu_surface_metrics.py)
# (the connected-component kernels of components.h — cc_tile_kernel<uint8 | int64, 1 | 2 | 3>, cc_merge_kernel<uint8 | int64, 1 | 2 | 3>,
#  cc_flatten_kernel, cc_reduce_kernel<uint8 | int64>, cc_finish_kernel, cc_filter_kernel<uint8 | int64> — are launched by
#  tests/test_gpu_components.py: test_case and test_scattered_prediction_64x80x72 run both element sizes under each connectivity)
# (the live batch of the upper decoder's backward, DESIGN.md §4.4, adds no kernel: its launches are the same kernels on fewer samples plus
#  fill nodes; maxpool2_bwd_add_kernel / maxpool2_bwd_add_x2_kernel gained one argument — tests/test_gpu_live_batch.py runs both sides of it)
# (crop_rotflip_channels_kernel<1> and <4>, channel_norm_partial_kernel<1> and <2>, channel_norm_finish_kernel<1> and <2>,
#  channel_norm_apply_kernel<1> and <4> of datafeed.h, the multi-modal feed and its channel-wise normalisation, are launched by
#  tests/test_gpu_multimodal.py: the (6, 6, 5) and (6, 6, 8) sweeps at 1..4 channels, and the (3, 5, 7, 9) / misaligned volumes for the
#  one-voxel kernels, (3, 5, 6, 8) and (3, 24, 40, 41) for the quad kernels of the normalisation)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/cov
rm -rf $O; mkdir -p $O
cd $R
rocprofv3 --kernel-trace --stats -d $O/suite -o c --output-format csv -- python3 -m pytest tests -m gpu -q -p no:cacheprovider > $O/suite.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/unet -o c --output-format csv -- python3 bench.py --full --steps 3 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --stats -d $O/unet16 -o c --output-format csv -- python3 bench.py --full --num-classes 16 --steps 3 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --stats -d $O/swin -o c --output-format csv -- python3 bench.py --full --model swinunetr_icl --steps 3 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --stats -d $O/refloop -o c --output-format csv -- python3 bench.py --full --loop reference --steps 3 --warmup 2 > /dev/null 2>&1
python3 tools/kernel_coverage.py $O > $R/gpurun_out/kernel_coverage.txt 2>&1
tail -2 $O/suite.log
find $O -name '*kernel_trace.csv' -delete      # tens of MB each; the stats CSVs are what the summary reads
