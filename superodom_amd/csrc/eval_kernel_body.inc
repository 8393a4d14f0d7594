// eval_kernel_body.inc -- the body of eval_kernel and of eval_kernel_prior (kernels.hip), included once for each with
//   SO_BODY_KERNEL  the kernel's own instantiation (its kernarg lines)
//   SO_BODY_PRIOR   false / true: eval_pass without / with the pose prior
//   SO_BODY_PRIOR_WORDS   nullptr / the prior's 55 doubles (the kernel's last argument)
// One text, two kernels of different names: a registration without a prior launches the functions it always launched.
  __shared__ EvalShared sh;
  if (SO_ENTRY_WARM) {
    st = after_loaded(st, kernarg_lines<decltype(&SO_BODY_KERNEL)>());
    st = after_loaded(st, SO_WARM_FIELDS(st, DevState, max_outer, eval_pose));  // reg_done, lm_more, either pose
  }
  if (!eval_slot_active(st, slot)) return;
  const Pose pose = pose_from_array(slot == 0 ? st->T : st->eval_pose);
  (void)eval_pass<FIT, false, PROF, false, false, SO_BODY_PRIOR>(slot, fuse_lm, pose, spx, spy, spz, corr, st, ep, partials, ticket, hist, out, mpts, nbr5, mp, sh, SO_BODY_PRIOR_WORDS);
