"""``Visualizer``: the reference's ``util/visualizer.py`` -- pictures of a training run under
``checkpoints_dir/name/web`` with a self-refreshing ``index.html``, the ``loss_log.txt`` lines, and ``save_images`` for the
test drivers' result pages.  File names, the page layout and the log format are upstream's.  The TensorFlow-1 summary
writer behind ``--tf_log`` is not carried over: asking for it raises."""
import ntpath
import os
import time

from . import html
from . import util


class Visualizer(object):
    def __init__(self, opt):
        self.tf_log = opt.tf_log
        self.use_html = opt.isTrain and not opt.no_html
        self.win_size = opt.display_winsize
        self.name = opt.name
        if self.tf_log:
            raise NotImplementedError('--tf_log: the TensorFlow 1 summaries (tf.summary.FileWriter / tf.Summary) of the '
                                      'reference are not carried over; use the HTML page and loss_log.txt')
        if self.use_html:
            self.web_dir = os.path.join(opt.checkpoints_dir, opt.name, 'web')
            self.img_dir = os.path.join(self.web_dir, 'images')
            print('create web directory %s...' % self.web_dir)
            util.mkdirs([self.web_dir, self.img_dir])
        self.log_name = os.path.join(opt.checkpoints_dir, opt.name, 'loss_log.txt')
        util.mkdir(os.path.dirname(self.log_name))
        with open(self.log_name, 'a') as log_file:
            log_file.write('================ Training Loss (%s) ================\n' % time.strftime('%c'))

    @staticmethod
    def _entries(visuals, prefix):
        """(file name, caption) of every picture of ``visuals`` in order; a list entry contributes one per element."""
        out = []
        for label, image_numpy in visuals.items():
            if isinstance(image_numpy, list):
                out += [('%s_%s_%d.jpg' % (prefix, label, i), label + str(i), im) for i, im in enumerate(image_numpy)]
            else:
                out.append(('%s_%s.jpg' % (prefix, label), label, image_numpy))
        return out

    def display_current_results(self, visuals, epoch, step):
        """|visuals|: dictionary of pictures.  Saves them as epoch%.3d_<label>.jpg and rewrites the page, newest epoch
        first; ten or more pictures of an epoch are split into two rows."""
        if not self.use_html:
            return
        for name, _, image_numpy in self._entries(visuals, 'epoch%.3d' % epoch):
            util.save_image(image_numpy, os.path.join(self.img_dir, name))
        webpage = html.HTML(self.web_dir, 'Experiment name = %s' % self.name, refresh=5)
        for n in range(epoch, 0, -1):
            webpage.add_header('epoch [%d]' % n)
            entries = self._entries(visuals, 'epoch%.3d' % n)
            ims = [e[0] for e in entries]
            txts = [e[1] for e in entries]
            if len(ims) < 10:
                webpage.add_images(ims, txts, ims, width=self.win_size)
            else:
                num = int(round(len(ims) / 2.0))
                webpage.add_images(ims[:num], txts[:num], ims[:num], width=self.win_size)
                webpage.add_images(ims[num:], txts[num:], ims[num:], width=self.win_size)
        webpage.save()

    def plot_current_errors(self, errors, step):
        """Upstream writes TensorFlow scalars here when ``tf_log`` is on and does nothing otherwise."""
        return None

    def print_current_errors(self, epoch, i, errors, t):
        message = '(epoch: %d, iters: %d, time: %.3f) ' % (epoch, i, t)
        for k, v in errors.items():
            if v != 0:
                message += '%s: %.3f ' % (k, v)
        print(message)
        with open(self.log_name, 'a') as log_file:
            log_file.write('%s\n' % message)

    def save_images(self, webpage, visuals, image_path):
        """One header and one row on ``webpage`` for the example ``image_path[0]``: <its base name>_<label>.jpg each."""
        image_dir = webpage.get_image_dir()
        name = os.path.splitext(ntpath.basename(image_path[0]))[0]
        webpage.add_header(name)
        ims, txts = [], []
        for label, image_numpy in visuals.items():
            image_name = '%s_%s.jpg' % (name, label)
            util.save_image(image_numpy, os.path.join(image_dir, image_name))
            ims.append(image_name)
            txts.append(label)
        webpage.add_images(ims, txts, ims, width=self.win_size)
