/*
 * train_nn -- train a libhpnn network from a configuration file.
 *
 * Workflow parity with the reference CLI (tests/train_nn.c:59-255):
 *   init library -> parse flags -> load conf (generate or load weights)
 *   -> dump kernel.tmp (weights before training) -> nn_train_kernel
 *   -> dump kernel.opt (weights after training) -> deinit.
 * With -x (dry run) the two dumps are skipped.
 * Extension: -r STATE resumes exactly from STATE when it exists (weights bit-exact,
 * momentum, progress; see csrc/core/state.cpp) and writes it after training.
 */
#include <sys/stat.h>
#include <libhpnn.h>
#include "cli_common.h"

static void dump_help(void) {
    _OUT(stdout, "***********************************\n");
    _OUT(stdout, "usage:  train_nn [-options] [input]\n");
    _OUT(stdout, "***********************************\n");
    _OUT(stdout, "options:\n");
    _OUT(stdout, "-h \tdisplay this help;\n");
    _OUT(stdout, "-v \tincrease verbosity;\n");
    _OUT(stdout, "-x \tdry run (do not write kernel files).\n");
    _OUT(stdout, "-O N\thost threads.\n");
    _OUT(stdout, "-B N\tBLAS threads (accepted, unused).\n");
    _OUT(stdout, "-S N\tHIP streams per GPU.\n");
    _OUT(stdout, "-G N\tnumber of GPUs.\n");
    _OUT(stdout, "-b N\tminibatch size (batched mode).\n");
    _OUT(stdout, "-e N\tepochs (batched mode).\n");
    _OUT(stdout, "-m M\tmode: online | batched.\n");
    _OUT(stdout, "-d D\tdtype: f64 | f32 | bf16.\n");
    _OUT(stdout, "-l X\tlearning rate.  -a X momentum.\n");
    _OUT(stdout, "-c \tforce the CPU engine.\n");
    _OUT(stdout, "-R \treshuffle the samples every epoch (batched mode; [shuffle] epoch).\n");
    _OUT(stdout, "-V N\tvalidate on [test_dir] every N epochs and after the last (batched mode; [validate] N).\n");
    _OUT(stdout, "-K M\treturn the state of the best validation pass, M: loss | acc (needs -V; [keep_best]).\n");
    _OUT(stdout, "-P P\tstop after P validation passes without improvement (needs -K; [patience] P).\n");
    _OUT(stdout, "-L S\tlearning-rate schedule, S: constant | step | linear | plateau (batched mode; [lr_schedule]).\n");
    _OUT(stdout, "-C c\tclip the gradient of every step to the global L2 norm c (batched mode; [clip]).\n");
    _OUT(stdout, "-X F\tper-class validation metrics; the confusion matrix goes to F (needs -V; [confusion] on).\n");
    _OUT(stdout, "-r F\texact-resume state file (read if present, written after training).\n");
    _OUT(stdout, "-M F\tJSON-lines metrics file.  -T trace ranges + timing table.\n");
    _OUT(stdout, "***********************************\n");
    _OUT(stdout, "input: neural network conf file\n");
    _OUT(stdout, "(default ./nn.conf)\n");
    _OUT(stdout, "***********************************\n");
}

int main(int argc, char *argv[]) {
    cli_opts o;
    _NN(init, all)(0);
    if (cli_parse(argc, argv, &o, 1)) {
        dump_help();
        _NN(deinit, all)();
        return -1;
    }
    if (o.help) {
        dump_help();
        _NN(deinit, all)();
        return 0;
    }
    cli_apply_runtime(&o);
    nn_def *neural = _NN(load, conf)(o.conf);
    if (!neural) {
        _OUT(stderr, "FAILED to read NN configuration file! (ABORTING)\n");
        _NN(deinit, all)();
        return -1;
    }
    cli_apply_conf(&o, neural);
    struct stat st;
    if (o.state && stat(o.state, &st) == 0 && !_NN(load, state)(neural, o.state)) {
        _OUT(stderr, "FAILED to load state file %s! (ABORTING)\n", o.state);
        _NN(deinit, conf)(neural);
        free(neural);
        _NN(deinit, all)();
        return -1;
    }
    if (_NN(return, verbose)() > 1) _NN(dump, conf)(neural, stdout);
    /* rank 0 alone writes the kernel files (every rank holds the same weights; a second
     * fopen("w") of the same path would truncate rank 0's file) */
    UINT task = 0;
    _NN(get, curr_mpi_task)(&task);
    const bool writer = !_NN(return, dry)() && task == 0;
    /* HPNN_KERNEL_EXACT=1: kernel files with %.17g (bit-exact FP64 round trip) instead of
     * the reference's %17.15f -- parity tests compare weights below the text rounding */
    const char *ex = getenv("HPNN_KERNEL_EXACT");
    const bool exact = ex && ex[0] == '1';
    auto dump = [&](FILE *f) {
        if (exact) _NN(dump, kernel_exact)(neural, f);
        else _NN(dump, kernel)(neural, f);
    };
    if (writer) {
        FILE *f = fopen("./kernel.tmp", "w");
        if (!f) {
            _OUT(stderr, "FAILED to open kernel.tmp for writing!\n");
        } else {
            dump(f);
            fclose(f);
        }
    }
    BOOL ok = _NN(train, kernel)(neural);
    if (!ok) _OUT(stderr, "Training FAILED!\n");
    if (writer) {
        FILE *f = fopen("./kernel.opt", "w");
        if (!f) {
            _OUT(stderr, "FAILED to open kernel.opt for writing!\n");
        } else {
            dump(f);
            fclose(f);
        }
        if (o.state && ok && !_NN(dump, state)(neural, o.state)) ok = FALSE;
    }
    if (o.matrix && ok && task == 0 && cli_write_matrix(&o, neural)) ok = FALSE;
    if (hpnn_trace_enabled()) hpnn_trace_report(stdout);
    _NN(deinit, conf)(neural);
    free(neural);
    _NN(deinit, all)();
    return ok ? 0 : 1;
}
